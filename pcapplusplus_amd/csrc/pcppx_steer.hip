// pcppx_steer.hip — pcppx_steer_device: stable K-way partition of variable-length packets in HBM (flow steering).
//
// Packet i goes to bucket[i] (column mode) or key[i] % n_buckets (key mode); the output is bucket-major and stable:
// one radix pass of a counting sort whose payload is the packet bytes. Four plain launches in stream order; no block
// waits on another, and placement comes from counts and scans only (LDS atomics are used for sums, never for places):
//   steer_count_kernel    per kSteerBlockPk-packet block: packets and bytes per bucket (LDS histogram), written
//                         bucket-major into scratch (row k = bucket k's block sums), plus dropped / bad descriptors
//   steer_scan_kernel     one wave per bucket: its row's exclusive prefix in place, kSteerScanStep blocks a step with a
//                         running carry, and the bucket's totals
//   steer_bases_kernel    one wave: the K bucket totals -> bucket_first / bucket_pos, the totals, the overflow verdict
//   steer_copy_kernel     exits when the verdict is set. Else, per block: the four waves' own histograms -> each wave's
//                         running rank / byte position per bucket (LDS); then each wave takes its four 64-packet tiles one
//                         after another: a packet's stable rank and the bytes ahead of it among the tile's packets of its
//                         bucket (a 64-step lane walk), the descriptors, and the bytes: the tile's whole destination 16-B
//                         chunks as one flattened list walked over the 64 lanes (two aligned source granules funnel-shifted
//                         into one 16-B store), then every packet's own head and tail bytes
// All byte positions are 64-bit. Source bytes are read only through aligned 16-B granules that hold a byte of a steered
// packet; destination bytes only inside the packet's own span.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"

namespace pcppx
{
namespace
{
using namespace move;
constexpr uint32_t kStThreads = 256, kStWaves = kStThreads / 64;
constexpr uint32_t kStTilesPerWave = 4;
static_assert(kStWaves * kStTilesPerWave * 64 == kSteerBlockPk, "a block steers kSteerBlockPk packets");
static_assert(kSteerScanStep == 64, "one block sum per lane and step");
static_assert(PCPPX_STEER_MAX_BUCKETS <= kStThreads, "one thread per bucket");
constexpr uint32_t kStUnroll = 4;           // 16-B chunks a lane has in flight in the copy loop
constexpr uint32_t kNoBucket = 0xFFFFFFFFu;  // not steered: dropped, bad, or past the batch's end

struct StIn
{
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	uint64_t data_len;
	uint32_t n;
	const uint8_t* bucket;  // column mode, else null
	const uint8_t* key;     // key mode: packet 0's 32-bit key
	uint32_t key_stride;
	uint32_t n_buckets;
	uint32_t snaplen;
};

struct StOut
{
	uint8_t* data;  // null: index-only
	uint64_t data_cap;
	uint64_t* offsets;
	uint32_t* caplens;
	uint32_t* index;
	uint32_t* bucket_first;
	uint64_t* bucket_pos;
	uint32_t max_packets;
	uint64_t* totals;
};

// packet i's bucket (kNoBucket unless steered: off / len = its source offset and output length); drop: a column value
// >= n_buckets (its descriptor is not read); bad: a bucket, but offsets[i] + caplens[i] > data_len (never read)
__device__ __forceinline__ uint32_t classify(const StIn& p, uint64_t i, bool& drop, bool& bad, uint32_t& len,
                                             uint64_t& off)
{
	drop = bad = false;
	len = 0;
	off = 0;
	if (i >= p.n)
		return kNoBucket;
	const uint32_t v = p.bucket != nullptr ? (uint32_t)p.bucket[i]
	                                       : *reinterpret_cast<const uint32_t*>(p.key + i * p.key_stride) % p.n_buckets;
	if (v >= p.n_buckets)
	{
		drop = true;
		return kNoBucket;
	}
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, p.snaplen, i, off, len))
	{
		bad = true;
		return kNoBucket;
	}
	return v;
}

// cnt / bytes: rows of g block sums, row k = bucket k
__global__ __launch_bounds__(kStThreads) void steer_count_kernel(StIn p, uint32_t g, uint32_t* __restrict__ cnt,
                                                                 uint64_t* __restrict__ bytes,
                                                                 uint32_t* __restrict__ bdrop,
                                                                 uint32_t* __restrict__ bbad)
{
	__shared__ uint32_t s_c[PCPPX_STEER_MAX_BUCKETS];
	__shared__ unsigned long long s_b[PCPPX_STEER_MAX_BUCKETS];
	__shared__ uint32_t s_drop, s_bad;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	s_c[threadIdx.x] = 0;
	s_b[threadIdx.x] = 0;
	if (threadIdx.x == 0)
		s_drop = s_bad = 0;
	__syncthreads();
	uint32_t nd = 0, nb = 0;
#pragma unroll
	for (uint32_t u = 0; u < kStTilesPerWave; ++u)
	{
		bool drop, bad;
		uint32_t len;
		uint64_t off;
		const uint32_t b = classify(p, tile_first(kSteerBlockPk, w * kStTilesPerWave + u) + lane, drop, bad, len, off);
		if (b != kNoBucket)  // sums: the order in which the adds land does not show
		{
			atomicAdd(&s_c[b], 1u);
			atomicAdd(&s_b[b], (unsigned long long)len);
		}
		nd += __popcll(__ballot(drop));
		nb += __popcll(__ballot(bad));
	}
	if (lane == 0)
	{
		atomicAdd(&s_drop, nd);
		atomicAdd(&s_bad, nb);
	}
	__syncthreads();
	if (threadIdx.x < p.n_buckets)
	{
		cnt[(uint64_t)threadIdx.x * g + blockIdx.x] = s_c[threadIdx.x];
		bytes[(uint64_t)threadIdx.x * g + blockIdx.x] = s_b[threadIdx.x];
	}
	if (threadIdx.x == 0)
	{
		bdrop[blockIdx.x] = s_drop;
		bbad[blockIdx.x] = s_bad;
	}
}

// One wave per bucket (blockIdx.x): the exclusive prefix of its row of g block sums, in place, kSteerScanStep blocks a
// step (one per lane, a wave scan, a running carry; the next step's loads are in flight meanwhile), then its totals.
__global__ __launch_bounds__(64) void steer_scan_kernel(uint32_t g, uint32_t* __restrict__ cnt,
                                                        uint64_t* __restrict__ bytes, uint32_t* __restrict__ ktot_cnt,
                                                        uint64_t* __restrict__ ktot_bytes)
{
	const uint32_t lane = threadIdx.x;
	uint32_t* const rc = cnt + (uint64_t)blockIdx.x * g;
	uint64_t* const rb = bytes + (uint64_t)blockIdx.x * g;
	uint64_t run_c = 0, run_b = 0;
	uint64_t nc = lane < g ? rc[lane] : 0u, nb = lane < g ? rb[lane] : 0ull;
	for (uint32_t j0 = 0; j0 < g; j0 += kSteerScanStep)
	{
		const uint64_t c = nc, b = nb;
		const uint32_t j = j0 + lane, jn = j + kSteerScanStep;
		if (j0 + kSteerScanStep < g)
		{
			nc = jn < g ? rc[jn] : 0u;
			nb = jn < g ? rb[jn] : 0ull;
		}
		const uint64_t ic = wave_scan_incl(c, lane), ib = wave_scan_incl(b, lane);
		if (j < g)
		{
			rc[j] = (uint32_t)(run_c + ic - c);  // < the bucket's packets <= n
			rb[j] = run_b + ib - b;
		}
		run_c += __shfl(ic, 63);
		run_b += __shfl(ib, 63);
	}
	if (lane == 0)
	{
		ktot_cnt[blockIdx.x] = (uint32_t)run_c;
		ktot_bytes[blockIdx.x] = run_b;
	}
}

// One wave: the K bucket totals -> bucket_first / bucket_pos (64 buckets a step), the dropped / bad sums over the g
// blocks (64 a step), the totals and the all-or-nothing overflow verdict the copy kernel reads.
__global__ __launch_bounds__(64) void steer_bases_kernel(uint32_t g, uint32_t K, const uint32_t* __restrict__ ktot_cnt,
                                                         const uint64_t* __restrict__ ktot_bytes,
                                                         const uint32_t* __restrict__ bdrop,
                                                         const uint32_t* __restrict__ bbad, StOut o)
{
	const uint32_t lane = threadIdx.x;
	uint64_t run_c = 0, run_b = 0;
	for (uint32_t k0 = 0; k0 < K; k0 += 64)
	{
		const uint32_t k = k0 + lane;
		const uint64_t c = k < K ? ktot_cnt[k] : 0u, b = k < K ? ktot_bytes[k] : 0ull;
		const uint64_t ic = wave_scan_incl(c, lane), ib = wave_scan_incl(b, lane);
		if (k < K)
		{
			o.bucket_first[k] = (uint32_t)(run_c + ic - c);
			o.bucket_pos[k] = run_b + ib - b;
		}
		run_c += __shfl(ic, 63);
		run_b += __shfl(ib, 63);
	}
	uint64_t drop = 0, bad = 0;
#pragma unroll 8  // independent loads: eight steps' worth in flight
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
		drop += j < g ? bdrop[j] : 0u;
		bad += j < g ? bbad[j] : 0u;
	}
	drop = wave_sum(drop);
	bad = wave_sum(bad);
	if (lane == 0)
	{
		o.bucket_first[K] = (uint32_t)run_c;
		o.bucket_pos[K] = run_b;
		o.totals[PCPPX_STEER_STEERED_PACKETS] = run_c;
		o.totals[PCPPX_STEER_STEERED_BYTES] = run_b;
		o.totals[PCPPX_STEER_DROPPED] = drop;
		o.totals[PCPPX_STEER_BAD_DESC] = bad;
		o.totals[PCPPX_STEER_OVERFLOW] = (run_c > o.max_packets || (o.data != nullptr && run_b > o.data_cap)) ? 1 : 0;
		o.totals[5] = o.totals[6] = o.totals[7] = 0;
	}
}

__global__ __launch_bounds__(kStThreads) void steer_copy_kernel(StIn p, StOut o, uint32_t g,
                                                                const uint32_t* __restrict__ cnt,
                                                                const uint64_t* __restrict__ bytes)
{
	// per wave and bucket: the rank and byte position of the wave's next packet of that bucket
	__shared__ uint32_t s_rc[kStWaves][PCPPX_STEER_MAX_BUCKETS];
	__shared__ unsigned long long s_rb[kStWaves][PCPPX_STEER_MAX_BUCKETS];
	// per wave, for the tile it is moving, per packet (lane): the exclusive prefix of the whole-chunk counts (one more
	// entry for their sum), the destination and source positions (shifted so that position % 16 = address % 16)
	__shared__ uint64_t s_cp[kStWaves][65];
	__shared__ uint64_t s_dq[kStWaves][64];
	__shared__ uint64_t s_sa[kStWaves][64];
	if (o.totals[PCPPX_STEER_OVERFLOW] != 0)  // all or nothing: the same word for every block
		return;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
	for (uint32_t x = 0; x < kStWaves; ++x)
	{
		s_rc[x][threadIdx.x] = 0;
		s_rb[x][threadIdx.x] = 0;
	}
	__syncthreads();
#pragma unroll
	for (uint32_t u = 0; u < kStTilesPerWave; ++u)
	{
		bool drop, bad;
		uint32_t len;
		uint64_t off;
		const uint32_t b = classify(p, tile_first(kSteerBlockPk, w * kStTilesPerWave + u) + lane, drop, bad, len, off);
		if (b != kNoBucket)
		{
			atomicAdd(&s_rc[w][b], 1u);
			atomicAdd(&s_rb[w][b], (unsigned long long)len);
		}
	}
	__syncthreads();
	if (threadIdx.x < p.n_buckets)  // bucket k: behind the buckets before it, the blocks before this one, the waves before
	{
		const uint32_t k = threadIdx.x;
		uint32_t c = o.bucket_first[k] + cnt[(uint64_t)k * g + blockIdx.x];
		uint64_t b = o.bucket_pos[k] + bytes[(uint64_t)k * g + blockIdx.x];
#pragma unroll
		for (uint32_t x = 0; x < kStWaves; ++x)
		{
			const uint32_t tc = s_rc[x][k];
			const uint64_t tb = s_rb[x][k];
			s_rc[x][k] = c;
			s_rb[x][k] = b;
			c += tc;
			b += tb;
		}
	}
	__syncthreads();
	const bool copy = o.data != nullptr;
	const auto [dbase, dal] = align16(o.data);  // position q (= byte position + dal) lives at dbase + q
	const auto [sbase, sal] = align16(p.data);  // the same for source positions (= batch offset + sal)
	uint64_t* const cp = s_cp[w];
	uint64_t* const dq = s_dq[w];
	uint64_t* const sa = s_sa[w];

#pragma unroll 1
	for (uint32_t u = 0; u < kStTilesPerWave; ++u)
	{
		const uint64_t i = tile_first(kSteerBlockPk, w * kStTilesPerWave + u) + lane;
		bool drop, bad;
		uint32_t len;
		uint64_t off;
		const uint32_t b = classify(p, i, drop, bad, len, off);  // the descriptors again (cache hits)
		if (__ballot(b != kNoBucket) == 0)
			continue;
		// among the tile's packets of this lane's bucket: how many, and how many bytes, lie ahead of it, and is it the last
		uint32_t rank = 0;
		uint64_t before = 0;
		bool last = true;
#pragma unroll 4
		for (uint32_t j = 0; j < 64; ++j)
		{
			const uint32_t bj = __builtin_amdgcn_readlane(b, j), lj = __builtin_amdgcn_readlane(len, j);
			const bool same = bj == b;
			rank += (same && j < lane) ? 1u : 0u;
			before += (same && j < lane) ? lj : 0u;
			last = last && !(same && j > lane);
		}
		const bool st = b != kNoBucket;
		// the wave's own LDS rows: its LDS accesses complete in program order, so a wave-level fence (no block barrier:
		// the waves' tiles differ) orders these accesses behind the previous tile's
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		const uint32_t r = st ? s_rc[w][b] + rank : 0u;
		const uint64_t pos = st ? s_rb[w][b] + before : 0ull;
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		if (st && last)  // one lane per bucket: the next tile's packets of the bucket go behind this one
		{
			s_rc[w][b] = r + 1;
			s_rb[w][b] = pos + len;
		}
		if (st)
		{
			o.offsets[r] = pos;
			o.caplens[r] = len;
			if (o.index != nullptr)
				o.index[r] = (uint32_t)i;
		}
		if (!copy)  // index-only (uniform over the grid)
			continue;
		// the packet's destination span [q, e): a head up to the first 16-B boundary, whole chunks, a tail
		const uint64_t q = pos + dal, e = q + len, s0 = off + sal;
		const uint64_t up = (q + 15) & ~15ull;
		const uint64_t he = e < up ? e : up;                   // head [q, he)
		const uint64_t dn = e & ~15ull, ts = dn > he ? dn : he;  // tail [ts, e)
		const uint64_t nfull = (st && dn > up) ? (dn - up) >> 4 : 0ull;
		const uint64_t incl = wave_scan_incl(nfull, lane);
		cp[lane] = incl - nfull;
		if (lane == 63)
			cp[64] = incl;
		dq[lane] = up;             // the first whole chunk
		sa[lane] = s0 + (up - q);  // and its source position
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		const uint64_t total = cp[64];
		for (uint64_t c0 = 0; c0 < total; c0 += 64 * kStUnroll)
		{
			// kStUnroll chunks per lane, 64 chunks apart. Each chunk's two aligned source granules (the second one only
			// when the source is not aligned like the destination, else the first one again) are loaded unconditionally,
			// so all loads are in flight together; a chunk past the list's end loads the last chunk's again.
			uint64_t s[kStUnroll], cs[kStUnroll];
			uint32_t live = 0;
#pragma unroll
			for (uint32_t x = 0; x < kStUnroll; ++x)
			{
				const uint64_t c = c0 + 64 * x + lane;
				live |= (c < total ? 1u : 0u) << x;
				const uint64_t cc = c < total ? c : total - 1;
				const uint32_t k = find_packet(cp, cc);
				const uint64_t ahead = (cc - cp[k]) << 4;
				cs[x] = dq[k] + ahead;
				s[x] = sa[k] + ahead;
			}
			uint4 a[kStUnroll], bb[kStUnroll];
#pragma unroll
			for (uint32_t x = 0; x < kStUnroll; ++x)
			{
				const uint4* gp = reinterpret_cast<const uint4*>(sbase + (s[x] & ~15ull));
				a[x] = gp[0];
				bb[x] = gp[(s[x] & 15) != 0 ? 1 : 0];
			}
#pragma unroll
			for (uint32_t x = 0; x < kStUnroll; ++x)
				if ((live >> x) & 1)
					*reinterpret_cast<uint4*>(dbase + cs[x]) = funnel16(a[x], bb[x], (uint32_t)(s[x] & 15));
		}
		// each packet's own head and tail bytes (fewer than 16 each): no chunk is shared between packets
		copy_edge(sbase, dbase, s0, q, st ? (uint32_t)(he - q) : 0u);
		copy_edge(sbase, dbase, s0 + (ts - q), ts, st ? (uint32_t)(e - ts) : 0u);
	}
}
}  // namespace

uint32_t steer_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kSteerBlockPk - 1) / kSteerBlockPk);
}

uint64_t steer_scratch_bytes(uint32_t n, uint32_t n_buckets)
{
	const uint64_t g = steer_blocks(n), k = n_buckets;
	return 12 * k * g + 12 * k + 8 * g;
}

int launch_steer(const pcppx_batch* b, const pcppx_steer_spec* s, const pcppx_steering* out, void* scratch,
                 hipStream_t stream)
{
	const uint32_t g = steer_blocks(b->n), K = s->n_buckets;
	uint64_t* bytes = static_cast<uint64_t*>(scratch);  // K rows of g
	uint64_t* ktot_bytes = bytes + (uint64_t)K * g;
	uint32_t* cnt = reinterpret_cast<uint32_t*>(ktot_bytes + K);  // K rows of g
	uint32_t* ktot_cnt = cnt + (uint64_t)K * g;
	uint32_t* bdrop = ktot_cnt + K;
	uint32_t* bbad = bdrop + g;
	StIn in{ b->data,
		     b->offsets,
		     b->caplens,
		     b->data_len,
		     b->n,
		     s->bucket,
		     static_cast<const uint8_t*>(s->key),
		     s->key_stride,
		     K,
		     s->snaplen };
	StOut o{ out->data,         out->data_cap,   out->offsets,     out->caplens, out->index,
		     out->bucket_first, out->bucket_pos, out->max_packets, out->totals };
	hipLaunchKernelGGL(steer_count_kernel, dim3(g), dim3(kStThreads), 0, stream, in, g, cnt, bytes, bdrop, bbad);
	hipLaunchKernelGGL(steer_scan_kernel, dim3(K), dim3(64), 0, stream, g, cnt, bytes, ktot_cnt, ktot_bytes);
	hipLaunchKernelGGL(steer_bases_kernel, dim3(1), dim3(64), 0, stream, g, K, ktot_cnt, ktot_bytes, bdrop, bbad, o);
	hipLaunchKernelGGL(steer_copy_kernel, dim3(g), dim3(kStThreads), 0, stream, in, o, g, cnt, bytes);
	return check_launch("steer", stream);
}
}  // namespace pcppx
