// pcppx_bpf.hip — pcppx_bpf_device: classic BPF programs interpreted over the packets of a device batch.
//
// One lane per packet, one wave per 64-packet tile (a wave takes its block's tiles one after another when the batch
// has more chunks than the grid has blocks), one launch. The machine is the one include/pcppx.h states
// (libpcap's userland bpf_filter without auxiliary data); every lane keeps its own A, X and pc, and its 16 M[] words
// in its own column of the wave's [16][64] LDS block (the slot index comes from the instruction, so it is the same in
// every lane: one row, 64 consecutive dwords, no bank conflict, and no lane ever reads another lane's column).
//
// Instruction fetch is per wave, not per lane. The wave executes the instruction at `cur`, the lowest pc among its
// unfinished lanes, under the predicate pc == cur; the instruction word is read through a wave-uniform index, so the
// fetch and the whole opcode decode are scalar and the branches on the opcode are uniform. Jumps go forward only
// (the validator's rule), so cur rises strictly: every instruction is decoded at most once per wave whatever the
// divergence of the lanes, and a program ends within n_insns steps. The loop is bounded by n_insns on its own account
// as well, so that it ends over any buffer contents. After an instruction the next one is usually cur + 1 (some lane
// fell through: one ballot); only when no lane is there does the wave take the minimum over its lanes. The
// instruction at cur + 1 is fetched while the one at cur executes.
//
// Packet bytes are read through the aligned dword that holds the first byte and, when the value crosses into it, the
// next one (v_alignbyte, then a byte swap): never a word without a byte of the packet. All byte addresses are 64-bit.
// Several programs run one after another; lanes that have accepted sit out, and the wave stops when none is left.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"

namespace pcppx
{
namespace
{
constexpr uint32_t kBpfThreads = 256, kBpfWaves = kBpfThreads / 64;
// The grid's size limit: a block walks the batch's 256-packet chunks with the grid's stride and adds to the totals
// once. Measured on 10M IMIX packets: with one chunk per block the 39063 atomics per counter on one address
// cost 0.4 ms when every packet matches; with 2048 blocks (one resident set: 8 per CU) they cost nothing, but filters
// that read the packets run 1.4 x slower; 8192 keeps those within 5% of the unlimited grid at 0.03 ms for the atomics.
constexpr uint32_t kBpfMaxBlocks = 8192;
constexpr uint32_t kBpfDone = 0xFFFFFFFFu;  // pc of a lane that has returned, was rejected, or does not run

// instruction classes, and the fields of `code` (the BPF_* values of <pcap/bpf.h>)
constexpr uint32_t kLd = 0, kLdx = 1, kSt = 2, kStx = 3, kAlu = 4, kJmp = 5, kRet = 6;  // 7: MISC
constexpr uint32_t kImm = 0x00, kInd = 0x40, kMem = 0x60, kLen = 0x80, kMsh = 0xa0;
constexpr uint32_t kSizeH = 0x08, kSizeB = 0x10;
constexpr uint32_t kSrcX = 0x08, kRvalA = 0x10;
constexpr uint32_t kAdd = 0x00, kSub = 0x10, kMul = 0x20, kDiv = 0x30, kOr = 0x40, kAnd = 0x50, kLsh = 0x60, kRsh = 0x70,
                   kNeg = 0x80, kMod = 0x90, kXor = 0xa0;
constexpr uint32_t kJa = 0x00, kJeq = 0x10, kJgt = 0x20, kJge = 0x30;  // 0x40: JSET
constexpr uint32_t kTxa = 0x80;

struct BpfIn
{
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	const uint32_t* frame_lens;  // null: wirelen = caplen
	uint64_t data_len;
	uint32_t n;
};

struct BpfOut
{
	uint8_t* matched;
	uint8_t* bucket;
	uint32_t* ret;
	unsigned long long* totals;
};

// the lowest value over the wave's 64 lanes, as a scalar (called where the whole wave is active)
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
	for (int o = 32; o > 0; o >>= 1)
	{
		const uint32_t t = __shfl_xor(v, o);
		v = t < v ? t : v;
	}
	return __builtin_amdgcn_readfirstlane(v);
}

// the big-endian value of the `size` (1, 2 or 4) bytes at a: the aligned dword that holds a[0] and, only when the
// value reaches into it, the next one
__device__ __forceinline__ uint32_t load_be(const uint8_t* a, uint32_t size)
{
	const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(a) & 3);
	const uint32_t* w = reinterpret_cast<const uint32_t*>(a - sh);  // pointer arithmetic: the loads stay global loads
	const uint32_t w0 = w[0];
	const uint32_t w1 = w[sh + size > 4 ? 1 : 0];
	const uint32_t v = __builtin_amdgcn_alignbyte(w1, w0, sh);  // a[0] in the low byte
	return __builtin_bswap32(v) >> (32 - 8 * size);
}

__device__ __forceinline__ uint2 fetch(const pcppx_bpf_insn* insns, uint32_t at)
{
	return reinterpret_cast<const uint2*>(insns)[__builtin_amdgcn_readfirstlane(at)];
}

__global__ __launch_bounds__(kBpfThreads) void bpf_kernel(BpfIn p, BpfPrograms f, BpfOut o)
{
	__shared__ uint32_t s_m[kBpfWaves][PCPPX_BPF_MEMWORDS][64];
	__shared__ uint32_t s_cnt[2];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	if (threadIdx.x < 2)
		s_cnt[threadIdx.x] = 0;
	__syncthreads();
	uint32_t nm = 0, nb = 0;  // this wave's accepted packets and bad descriptors
	const uint64_t chunks = ((uint64_t)p.n + kBpfThreads - 1) / kBpfThreads;
#pragma unroll 1
	for (uint64_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x)  // the same trip count in all of a block's waves
	{
		const uint64_t i = chunk * kBpfThreads + threadIdx.x;
		const bool in = i < p.n;
		uint64_t off = 0;
		uint32_t buflen = 0, wirelen = 0;
		bool bad = false;
		if (in)
		{
			bad = move::out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, buflen);
			wirelen = p.frame_lens != nullptr ? p.frame_lens[i] : buflen;
		}
		const bool live = in && !bad;
		const uint8_t* const pkt = p.data + off;  // read only where live, at positions below buflen
		uint32_t(*const M)[64] = s_m[w];
		bool acc = false;
		uint32_t retv = 0, bkt = 0xFF;

#pragma unroll 1
		for (uint32_t q = 0; q < f.n_progs; ++q)
		{
			const bool run = live && !acc;
			if (__ballot(run) == 0)
				break;
			const uint32_t first = f.start[q], len = f.start[q + 1] - first;
			if ((f.uses_mem >> q) & 1)
			{
#pragma unroll
				for (uint32_t k = 0; k < PCPPX_BPF_MEMWORDS; ++k)
					M[k][lane] = 0;
			}
			uint32_t A = 0, X = 0, r = 0;
			uint32_t pc = run ? 0u : kBpfDone;
			uint32_t cur = 0;
			uint2 ins = fetch(f.insns, first);
#pragma unroll 1
			for (uint32_t step = 0; step < len; ++step)
			{
				const uint32_t ahead = cur + 1 < len ? cur + 1 : cur;
				const uint2 pre = fetch(f.insns, first + ahead);  // in flight while this instruction executes
				const bool on = pc == cur;
				const uint32_t code = ins.x & 0xFFFFu, jt = (ins.x >> 16) & 0xFFu, jf = ins.x >> 24, k = ins.y;
				uint32_t next = cur + 1;
				bool rej = false, fin = false;
				switch (code & 7u)
				{
				case kLd:
				case kLdx:
				{
					const uint32_t mode = code & 0xE0u;
					uint32_t v = 0;
					if (mode == kImm)
						v = k;
					else if (mode == kMem)
						v = M[k & (PCPPX_BPF_MEMWORDS - 1)][lane];
					else if (mode == kLen)
						v = wirelen;
					else  // a packet load: ABS (0x20), IND or MSH
					{
						const uint32_t size = (code & kSizeB) ? 1u : (code & kSizeH) ? 2u : 4u;
						const uint32_t x = mode == kInd ? X : 0u;
						// k > buflen || x > buflen - k || size > buflen - (x + k): nothing wraps
						const bool fits = k <= buflen && x <= buflen - k && size <= buflen - (x + k);
						rej = !fits;
						if (on && fits)
							v = load_be(pkt + (uint64_t)(x + k), size);
						if (mode == kMsh)
							v = (v & 0xFu) << 2;
					}
					if ((code & 7u) == kLdx)
						X = on && !rej ? v : X;
					else
						A = on && !rej ? v : A;
					break;
				}
				case kSt:
				case kStx:
					if (on)
						M[k & (PCPPX_BPF_MEMWORDS - 1)][lane] = (code & 7u) == kSt ? A : X;
					break;
				case kAlu:
				{
					const uint32_t s = (code & kSrcX) ? X : k;
					uint32_t v = A;
					switch (code & 0xF0u)
					{
					case kAdd: v = A + s; break;
					case kSub: v = A - s; break;
					case kMul: v = A * s; break;
					case kDiv: rej = s == 0; v = A / (s != 0 ? s : 1u); break;
					case kMod: rej = s == 0; v = A % (s != 0 ? s : 1u); break;
					case kOr: v = A | s; break;
					case kAnd: v = A & s; break;
					case kXor: v = A ^ s; break;
					case kLsh: v = s < 32 ? A << s : 0u; break;
					case kRsh: v = s < 32 ? A >> s : 0u; break;
					case kNeg: v = 0u - A; break;
					default: break;
					}
					A = on && !rej ? v : A;
					break;
				}
				case kJmp:
				{
					const uint32_t s = (code & kSrcX) ? X : k;
					const uint32_t op = code & 0xF0u;
					if (op == kJa)
						next = cur + 1 + k;
					else
					{
						const bool c = op == kJeq ? A == s : op == kJgt ? A > s : op == kJge ? A >= s : (A & s) != 0;
						next = cur + 1 + (c ? jt : jf);
					}
					break;
				}
				case kRet:
					fin = true;
					r = on ? ((code & 0x18u) == kRvalA ? A : k) : r;
					break;
				default:  // MISC
					if ((code & 0xF8u) == kTxa)
						A = on ? X : A;
					else
						X = on ? A : X;
					break;
				}
				if (on)
					pc = (rej || fin) ? kBpfDone : next;
				// the next instruction: usually the one behind this one, else the lowest pc left in the wave
				cur = cur + 1;
				if (__ballot(pc == cur) != 0)
					ins = pre;
				else
				{
					cur = wave_min(pc);
					if (cur >= len)  // every lane is done (or, over a corrupted buffer, out of the program)
						break;
					ins = fetch(f.insns, first + cur);
				}
			}
			if (run && r != 0)  // a lane that did not reach a RET has r == 0
			{
				acc = true;
				retv = r;
				bkt = q;
			}
		}

		if (in)
		{
			if (o.matched != nullptr)
				o.matched[i] = acc ? 1 : 0;
			if (o.bucket != nullptr)
				o.bucket[i] = (uint8_t)bkt;
			if (o.ret != nullptr)
				o.ret[i] = retv;
		}
		nm += (uint32_t)__popcll(__ballot(acc));
		nb += (uint32_t)__popcll(__ballot(in && bad));
	}
	if (lane == 0)
	{
		atomicAdd(&s_cnt[0], nm);
		atomicAdd(&s_cnt[1], nb);
	}
	__syncthreads();
	if (threadIdx.x < 2 && s_cnt[threadIdx.x] != 0)  // integer sums: the order in which they land does not show
		atomicAdd(&o.totals[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}
}  // namespace

int launch_bpf(const pcppx_batch* b, const uint32_t* frame_lens, const BpfPrograms& progs, const pcppx_bpf_verdicts* out,
               hipStream_t stream)
{
	static_assert(PCPPX_BPF_MATCHED == 0 && PCPPX_BPF_BAD_DESC == 1, "the block's two counters are totals[0] and [1]");
	static_assert(sizeof(pcppx_bpf_insn) == 8, "an instruction is fetched as one 8-byte word");
	const uint64_t chunks = ((uint64_t)b->n + kBpfThreads - 1) / kBpfThreads;
	const uint32_t g = (uint32_t)(chunks < kBpfMaxBlocks ? chunks : kBpfMaxBlocks);
	BpfIn in{ b->data, b->offsets, b->caplens, frame_lens, b->data_len, b->n };
	BpfOut o{ out->matched, out->bucket, out->ret, reinterpret_cast<unsigned long long*>(out->totals) };
	hipLaunchKernelGGL(bpf_kernel, dim3(g), dim3(kBpfThreads), 0, stream, in, progs, o);
	return check_launch("bpf", stream);
}
}  // namespace pcppx
