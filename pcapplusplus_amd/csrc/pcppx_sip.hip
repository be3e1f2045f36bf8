// pcppx_sip.hip — pcppx_sip_device: the SIP messages, their header fields and their SDP bodies of a batch in HBM.
//
// The contract is in include/pcppx.h (sip); the dispatch, the first lines, the field walk and the SDP body are
// pcppx_sip.h's, which pcppx_sip_ref.cpp compiles for the host. Plain launches in stream order; no block waits on
// another, no thread spins, no atomics. Every grid is sized from n: a block owns kSipBlockPk source packets and their
// records. The shape is pcppx_http.hip's:
//   sip_plan_kernel  a thread per source packet, 1024 a block: the disposition from the descriptor, the recorded
//                    carrier and the payload's first bytes (rules 1-8); a message's thread does the whole walk with the
//                    counting sink (its field records, its text bytes, its header length, its linked fields, whether an
//                    SDP body follows). A 16-byte plan per packet; eleven 32-bit sums per block.
//   sip_base_kernel  one wave: exclusive prefixes of the blocks' messages, records, text bytes and SDP records, the
//                    totals, the all-or-nothing verdict
//   sip_emit_kernel  exits on overflow. The block's plans with the exclusive prefixes of their messages, records, text
//                    bytes and SDP records go to LDS; the disposition per source packet. The block's messages are
//                    listed densely in LDS, and thread h takes message h of the list (full waves where the SIP share
//                    is low): the walk again with the emitting sink, the SDP body's walk and its 32-byte record, then
//                    the 48-byte message record.
// A block is 1024 threads (16 waves, a wave per 64-packet tile) so that neither kernel loops around the walk. The spec
// (272 bytes) is copied to LDS first, so that the name comparison indexes LDS and not a register array.
// All byte positions are 64-bit. Source bytes are read only inside the carrier's payload of an in-bounds packet, plus
// the carrier header's port bytes and its last byte (rule 14).
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"
#include "pcppx_sip.h"

namespace pcppx
{
namespace
{
using namespace move;
using namespace sip;
constexpr uint32_t kSpThreads = kSipBlockPk, kSpWaves = kSpThreads / 64;  // a thread per packet, a wave per tile
static_assert(kSpThreads == 1024, "the largest block");
static_assert(kSipBlockPk <= 65536, "s_list holds 16-bit slots");
// a block's records, text bytes and header bytes fit 32 bits: each at most 65535 per packet
static_assert((uint64_t)kSipBlockPk * 65535 < (1ull << 32), "32-bit block sums");
constexpr uint32_t kNone = 0xFF;  // a plan's disp past the batch's end (never stored)
// messages, records, text bytes, SDP records, requests, responses, host, bad, header bytes, fields, heuristic
constexpr uint32_t kSpSums = 11, kSpBases = 4;
constexpr uint32_t kSpecWords = sizeof(pcppx_sip_spec) / 4;
static_assert(sizeof(pcppx_sip_spec) % 4 == 0, "copied to LDS by words");
constexpr uint32_t kBitVia = 1, kBitTcp = 2, kBitSdp = 4;  // Plan::bits

// What the emit kernel needs of a source packet, 16 bytes. All but disp: of a message only.
struct Plan
{
	uint16_t off, L;  // the layer
	uint16_t n_rec, text_len;
	uint16_t header_len, n_fields;
	uint8_t kind;
	uint8_t disp;  // PCPPX_SIP_* or kNone
	uint8_t bits;  // kBit*
	uint8_t pad;
};
static_assert(sizeof(Plan) == 16, "sip_scratch_bytes");

struct SpIn
{
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	uint64_t data_len;
	uint32_t n;
	const pcppx_layer* layers;
	uint32_t ml;
	const uint8_t* rec0;  // packet 0's summary or brief: flags at byte 12, n_layers at byte 14
	uint32_t rec_stride;
};

struct SpOut
{
	pcppx_sip_msg* msgs;
	pcppx_sip_field* fields;
	pcppx_sip_sdp* sdps;
	uint8_t* text;  // null: no text
	uint64_t text_cap;
	uint8_t* disposition;
	uint32_t max_msgs, max_fields, max_sdps, spec_msgs;  // spec_msgs: resolved (never 0 with n > 0)
	uint64_t* totals;
};

// the spec from the kernel's arguments to LDS, a word a thread; the caller synchronises
__device__ __forceinline__ void stage_spec(const pcppx_sip_spec& spec, uint32_t* s_spec)
{
	if (threadIdx.x < kSpecWords)
		s_spec[threadIdx.x] = reinterpret_cast<const uint32_t*>(&spec)[threadIdx.x];
}

// Packet i's plan (disp kNone past the batch's end).
__device__ __forceinline__ Plan classify(const SpIn& p, const pcppx_sip_spec* spec, uint64_t i)
{
	Plan pl{};
	pl.disp = kNone;
	if (i >= p.n)
		return pl;
	uint64_t off;
	uint32_t cap;
	pl.disp = PCPPX_SIP_BAD_DESC;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return pl;
	const uint8_t* rec = p.rec0 + i * p.rec_stride;
	const uint32_t flags = *reinterpret_cast<const uint16_t*>(rec + 12), n_layers = rec[14];
	const Layer l = find_layer(p.data + off, cap, p.layers + i * p.ml, n_layers, p.ml, flags, spec->kinds);
	pl.disp = (uint8_t)l.disp;
	if (l.disp != PCPPX_SIP_MSG)
		return pl;
	CountSink count;
	const Walk w = walk(p.data + off + l.off, l, spec, count);
	pl.off = (uint16_t)l.off;
	pl.L = (uint16_t)l.L;
	pl.kind = (uint8_t)l.kind;
	pl.bits = (uint8_t)((l.via != 0 ? kBitVia : 0) | (l.tcp != 0 ? kBitTcp : 0) |
	                    ((w.flags & PCPPX_SIP_HAS_SDP) != 0 ? kBitSdp : 0));
	pl.n_rec = (uint16_t)w.n_rec;
	pl.text_len = (uint16_t)w.text_len;
	pl.header_len = (uint16_t)w.header_len;
	pl.n_fields = (uint16_t)w.n_fields;
	return pl;
}

__global__ __launch_bounds__(kSpThreads) void sip_plan_kernel(SpIn p, pcppx_sip_spec spec, Plan* __restrict__ plan,
                                                              uint32_t* __restrict__ bsums)
{
	__shared__ uint32_t lc[kSpWaves][kSpSums];
	__shared__ uint32_t s_spec[kSpecWords];
	stage_spec(spec, s_spec);
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t i = tile_first(kSipBlockPk, w) + lane;
	const Plan pl = classify(p, reinterpret_cast<const pcppx_sip_spec*>(s_spec), i);
	if (pl.disp != kNone)
		plan[i] = pl;
	const bool m = pl.disp == PCPPX_SIP_MSG;
	// the tile's sums: 64 packets of at most 65535 each
	const uint64_t s01 = wave_sum((m ? 1u : 0u) | ((uint64_t)(m ? pl.n_rec : 0u) << 32));
	const uint64_t s28 = wave_sum((m ? pl.text_len : 0u) | ((uint64_t)(m ? pl.header_len : 0u) << 32));
	const uint64_t s45 = wave_sum((m && pl.kind == 0 ? 1u : 0u) | ((uint64_t)(m && pl.kind == 1 ? 1u : 0u) << 32));
	const uint64_t s67 = wave_sum((pl.disp == PCPPX_SIP_HOST ? 1u : 0u) |
	                              ((uint64_t)(pl.disp == PCPPX_SIP_BAD_DESC ? 1u : 0u) << 32));
	const uint64_t s3a = wave_sum((m && (pl.bits & kBitSdp) != 0 ? 1u : 0u) |
	                              ((uint64_t)(m && (pl.bits & kBitVia) != 0 ? 1u : 0u) << 32));
	const uint64_t s9 = wave_sum(m ? pl.n_fields : 0u);
	if (lane == 0)
	{
		lc[w][0] = (uint32_t)s01;
		lc[w][1] = (uint32_t)(s01 >> 32);
		lc[w][2] = (uint32_t)s28;
		lc[w][3] = (uint32_t)s3a;
		lc[w][4] = (uint32_t)s45;
		lc[w][5] = (uint32_t)(s45 >> 32);
		lc[w][6] = (uint32_t)s67;
		lc[w][7] = (uint32_t)(s67 >> 32);
		lc[w][8] = (uint32_t)(s28 >> 32);
		lc[w][9] = (uint32_t)s9;
		lc[w][10] = (uint32_t)(s3a >> 32);
	}
	__syncthreads();
	if (threadIdx.x < kSpSums)
	{
		const uint32_t k = threadIdx.x;
		uint32_t sum = 0;
		for (uint32_t x = 0; x < kSpWaves; ++x)
			sum += lc[x][k];
		bsums[(uint64_t)k * gridDim.x + blockIdx.x] = sum;
	}
}

// One wave: the exclusive prefixes of the g blocks' messages, records, text bytes and SDP records (64 a step, a running
// carry), the totals, the verdict. base: four arrays of g.
__global__ __launch_bounds__(64) void sip_base_kernel(uint32_t g, const uint32_t* __restrict__ bsums,
                                                      uint64_t* __restrict__ base, SpOut o)
{
	constexpr uint32_t kRest = kSpSums - kSpBases;
	const uint32_t lane = threadIdx.x;
	uint64_t run[kSpBases] = {}, sums[kRest] = {};
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
#pragma unroll
		for (uint32_t k = 0; k < kSpBases; ++k)
		{
			const uint64_t v = j < g ? bsums[(uint64_t)k * g + j] : 0u;
			const uint64_t iv = wave_scan_incl(v, lane);
			if (j < g)
				base[(uint64_t)k * g + j] = run[k] + iv - v;
			run[k] += __shfl(iv, 63);
		}
#pragma unroll
		for (uint32_t k = 0; k < kRest; ++k)
			sums[k] += j < g ? bsums[(uint64_t)(k + kSpBases) * g + j] : 0u;
	}
#pragma unroll
	for (uint32_t k = 0; k < kRest; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		o.totals[PCPPX_SIP_MSGS] = run[0];
		o.totals[PCPPX_SIP_REQUESTS] = sums[0];
		o.totals[PCPPX_SIP_RESPONSES] = sums[1];
		o.totals[PCPPX_SIP_FIELDS] = run[1];
		o.totals[PCPPX_SIP_TEXT_BYTES] = run[2];
		o.totals[PCPPX_SIP_HOST_N] = sums[2];
		o.totals[PCPPX_SIP_BAD_DESC_N] = sums[3];
		o.totals[PCPPX_SIP_HEADER_BYTES] = sums[4];
		o.totals[PCPPX_SIP_FIELDS_LINKED] = sums[5];
		o.totals[PCPPX_SIP_SDPS] = run[3];
		o.totals[PCPPX_SIP_BY_HEURISTIC] = sums[6];
		o.totals[PCPPX_SIP_OVERFLOW] = (run[0] > o.max_msgs || run[0] > o.spec_msgs || run[1] > o.max_fields ||
		                                run[3] > o.max_sdps || (o.text != nullptr && run[2] > o.text_cap))
		                                   ? 1
		                                   : 0;
	}
}

__global__ __launch_bounds__(kSpThreads) void sip_emit_kernel(SpIn p, pcppx_sip_spec spec, SpOut o,
                                                              const Plan* __restrict__ plan,
                                                              const uint64_t* __restrict__ base, uint32_t g)
{
	// 2 * (the tile's messages before the packet) + (the packet is a message), and from bit 16 the tile's SDP records
	// before the packet's
	__shared__ uint32_t s_cp[kSipBlockPk];
	__shared__ uint32_t s_rp[kSipBlockPk];  // the block's records before the packet's
	__shared__ uint32_t s_bp[kSipBlockPk];  // and its text bytes
	__shared__ uint32_t s_tc[kSpWaves], s_tr[kSpWaves], s_tb[kSpWaves], s_ts[kSpWaves];
	__shared__ uint32_t s_total;              // the block's messages
	__shared__ uint16_t s_list[kSipBlockPk];  // the block's messages: their slots, in source order
	__shared__ uint32_t s_spec[kSpecWords];
	if (o.totals[PCPPX_SIP_OVERFLOW] != 0)    // all or nothing: the same word for every block
		return;
	stage_spec(spec, s_spec);
	const uint32_t lane = threadIdx.x & 63, tl = threadIdx.x >> 6, slot = threadIdx.x;
	const uint64_t first = tile_first(kSipBlockPk, 0);
	{
		const uint64_t i = first + slot;
		uint32_t disp = kNone, rec = 0, bytes = 0, sdp = 0;
		if (i < p.n)
		{
			const Plan pl = plan[i];
			disp = pl.disp;
			rec = pl.n_rec;
			bytes = pl.text_len;
			sdp = (pl.bits & kBitSdp) != 0 ? 1 : 0;
			if (o.disposition != nullptr)
				o.disposition[i] = (uint8_t)disp;
		}
		const uint32_t cnt = disp == PCPPX_SIP_MSG ? 1 : 0;
		sdp &= cnt;
		// one scan for three: the tile's sums fit 7, 7 and 22 bits
		const uint64_t packed = cnt | (sdp << 8) | ((uint64_t)(cnt != 0 ? rec : 0u) << 16);
		const uint64_t ip = wave_scan_incl(packed, lane), ib = wave_scan_incl(cnt != 0 ? bytes : 0u, lane);
		const uint32_t ic = (uint32_t)(ip & 0xFF), is = (uint32_t)((ip >> 8) & 0xFF), ir = (uint32_t)(ip >> 16);
		s_cp[slot] = ((ic - cnt) << 1) | cnt | ((is - sdp) << 16);
		s_rp[slot] = ir - (cnt != 0 ? rec : 0u);
		s_bp[slot] = (uint32_t)ib - (cnt != 0 ? bytes : 0u);
		if (lane == 63)
		{
			s_tc[tl] = ic;
			s_tr[tl] = ir;
			s_tb[tl] = (uint32_t)ib;
			s_ts[tl] = is;
		}
	}
	__syncthreads();
	{
		uint32_t bc = 0, br = 0, bb = 0, bs = 0;
		for (uint32_t x = 0; x < tl; ++x)
		{
			bc += s_tc[x];
			br += s_tr[x];
			bb += s_tb[x];
			bs += s_ts[x];
		}
		const uint32_t v = s_cp[slot];
		s_rp[slot] += br;
		s_bp[slot] += bb;
		s_cp[slot] = v + (bs << 16);  // the block's SDP records before the packet's: at most 1024
		if ((v & 1) != 0)
			s_list[bc + ((v & 0xFFFF) >> 1)] = (uint16_t)slot;  // below the block's messages <= kSipBlockPk
		if (slot == kSipBlockPk - 1)
			s_total = bc + s_tc[tl];
	}
	__syncthreads();
	const uint32_t h = threadIdx.x;  // message h of the block's list
	if (h >= s_total)
		return;
	const uint64_t msg0 = base[blockIdx.x], rec0 = base[(uint64_t)g + blockIdx.x],
	               pos0 = base[2ull * g + blockIdx.x], sdp0 = base[3ull * g + blockIdx.x];
	const uint32_t mine = s_list[h];
	const uint64_t i = first + mine;  // < n: a message
	const Plan pl = plan[i];
	const Layer l{ PCPPX_SIP_MSG, pl.off, pl.L, pl.kind, (pl.bits & kBitVia) != 0 ? 1u : 0u,
		           (pl.bits & kBitTcp) != 0 ? 1u : 0u };
	const uint8_t* d = p.data + p.offsets[i] + pl.off;
	const uint64_t first_field = rec0 + s_rp[mine];  // first_field + n_rec <= FIELDS <= max_fields
	const uint64_t text_pos = pos0 + s_bp[mine];
	EmitSink sink{ o.fields + first_field, o.text, text_pos, (uint32_t)(msg0 + h) };
	const Walk wk = walk(d, l, reinterpret_cast<const pcppx_sip_spec*>(s_spec), sink);
	if ((pl.bits & kBitSdp) != 0)  // the plan's verdict: the same walk over the same bytes
	{
		const uint32_t body = pl.header_len, len = (uint32_t)pl.L - pl.header_len;
		const Sdp x = sdp_of(d + body, len);
		// sdp0 + ... < SDPS <= max_sdps
		put_sdp(o.sdps + (sdp0 + (s_cp[mine] >> 16)), (uint32_t)(msg0 + h), (uint32_t)i, body, len, x);
	}
	put_msg(o.msgs + (msg0 + h), first_field, text_pos, (uint32_t)i, l, wk);  // msg0 + h < MSGS <= max_msgs
}
}  // namespace

uint32_t sip_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kSipBlockPk - 1) / kSipBlockPk);
}

uint64_t sip_scratch_bytes(uint32_t n)
{
	return 76ull * sip_blocks(n) + 16ull * n;
}

int launch_sip(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
               const pcppx_sip_spec* spec, const pcppx_sip_out* out, void* scratch, hipStream_t stream)
{
	const uint32_t g = sip_blocks(b->n);
	// plan[n] | the exclusive prefixes of messages, records, text bytes, SDP records [g each, 64-bit] | eleven sums
	// [g each, 32-bit]: 16 n + 76 g bytes
	Plan* plan = static_cast<Plan*>(scratch);
	uint64_t* base = reinterpret_cast<uint64_t*>(plan + b->n);
	uint32_t* bsums = reinterpret_cast<uint32_t*>(base + (uint64_t)kSpBases * g);
	SpIn in{ b->data, b->offsets, b->caplens, b->data_len, b->n, layers, ml, rec0, rec_stride };
	SpOut o{ out->msgs,     out->fields,     out->sdps,     out->text,
		     out->text_cap, out->disposition, out->max_msgs, out->max_fields,
		     out->max_sdps, spec->max_msgs == 0 ? b->n : spec->max_msgs, out->totals };
	hipLaunchKernelGGL(sip_plan_kernel, dim3(g), dim3(kSpThreads), 0, stream, in, *spec, plan, bsums);
	hipLaunchKernelGGL(sip_base_kernel, dim3(1), dim3(64), 0, stream, g, bsums, base, o);
	hipLaunchKernelGGL(sip_emit_kernel, dim3(g), dim3(kSpThreads), 0, stream, in, *spec, o, plan, base, g);
	return check_launch("sip", stream);
}
}  // namespace pcppx
