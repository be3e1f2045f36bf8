// pcppx_select.hip — pcppx_select_device: stable stream compaction of variable-length packets in HBM.
//
// The packets a mask (keep[i] != 0) or a flags test ((flags[i] & flags_any) != 0) selects are gathered, in source
// order, into one packed batch: bytes back to back, offsets / caplens / source index per output packet, totals.
// Three plain launches in stream order (the dense_count_kernel / dense_copy_kernel shape); no block waits on another:
//   select_count_kernel  per 1024-packet block: selected packets, selected bytes (after snaplen), bad descriptors
//   select_base_kernel   one wave: exclusive prefix of the block sums (256 per step, running carry), the totals
//   select_copy_kernel   a block of 4 waves gathers 16 tiles of 64 packets, each wave its 4 tiles one after another:
//                        wave scan -> rank and byte position per packet, the tile's descriptors, then the tile's
//                        destination span walked in aligned 16-B chunks over the 64 lanes
// All byte positions are 64-bit. Source bytes are read only through aligned 16-B granules (or single bytes) that hold
// a byte of a selected, in-bounds packet; destination bytes only inside the span the tile owns.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"

namespace pcppx
{
namespace
{
using namespace move;
constexpr uint32_t kSelThreads = 256, kSelWaves = kSelThreads / 64;
constexpr uint32_t kSelTilesPerWave = 4, kSelTiles = kSelWaves * kSelTilesPerWave;  // 64-packet tiles per wave / block
static_assert(kSelTiles * 64 == kSelectBlockPk, "a block gathers kSelectBlockPk packets");
constexpr uint32_t kSelUnroll = 4;  // 16-B chunks a lane has in flight in the copy loop

struct SelIn
{
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	uint64_t data_len;
	uint32_t n;
	const uint8_t* keep;   // mask mode, else null
	const uint8_t* flags;  // flags mode: packet 0's 16-bit flags word
	uint32_t flags_stride;
	uint32_t flags_any;
	uint32_t invert;
	uint32_t snaplen;
};

struct SelOut
{
	uint8_t* data;  // null: index-only
	uint64_t data_cap;
	uint64_t* offsets;
	uint32_t* caplens;
	uint32_t* index;
	uint32_t max_packets;
	uint64_t* totals;
};

// packet i's verdict: sel (chosen and in bounds: off / len = its source offset and output length) or bad (chosen, but
// offsets[i] + caplens[i] > data_len). The descriptor of a packet the keep rule drops is not read.
__device__ __forceinline__ void classify(const SelIn& p, uint64_t i, bool& sel, bool& bad, uint32_t& len, uint64_t& off)
{
	sel = bad = false;
	len = 0;
	off = 0;
	if (i >= p.n)
		return;
	const bool chosen = p.keep != nullptr
	                        ? p.keep[i] != 0
	                        : (*reinterpret_cast<const uint16_t*>(p.flags + i * p.flags_stride) & p.flags_any) != 0;
	if (chosen == (p.invert != 0))
		return;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, p.snaplen, i, off, len))
	{
		bad = true;
		return;
	}
	sel = true;
}

__global__ __launch_bounds__(kSelThreads) void select_count_kernel(SelIn p, uint64_t* __restrict__ bbytes,
                                                                   uint32_t* __restrict__ bcnt,
                                                                   uint32_t* __restrict__ bbad)
{
	__shared__ uint64_t lb[kSelWaves];
	__shared__ uint32_t lc[kSelWaves], ld[kSelWaves];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t b = 0;
	uint32_t c = 0, d = 0;
#pragma unroll
	for (uint32_t u = 0; u < kSelTilesPerWave; ++u)
	{
		bool sel, bad;
		uint32_t len;
		uint64_t off;
		classify(p, tile_first(kSelectBlockPk, w * kSelTilesPerWave + u) + lane, sel, bad, len, off);
		b += len;
		c += __popcll(__ballot(sel));
		d += __popcll(__ballot(bad));
	}
	b = wave_sum(b);
	if (lane == 0)
	{
		lb[w] = b;
		lc[w] = c;
		ld[w] = d;
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		bbytes[blockIdx.x] = lb[0] + lb[1] + lb[2] + lb[3];
		bcnt[blockIdx.x] = lc[0] + lc[1] + lc[2] + lc[3];
		bbad[blockIdx.x] = ld[0] + ld[1] + ld[2] + ld[3];
	}
}

// One wave: the exclusive prefix of the g block sums, 256 at a step (four consecutive blocks per lane, one wave scan of
// the lanes' sums, a running carry; the next step's loads are in flight meanwhile), then the totals (the written counts
// are the selected ones unless the copy kernel finds the first selected packet that does not fit, which overwrites them).
__global__ __launch_bounds__(64) void select_base_kernel(uint32_t g, const uint64_t* __restrict__ bbytes,
                                                         const uint32_t* __restrict__ bcnt,
                                                         const uint32_t* __restrict__ bbad,
                                                         uint64_t* __restrict__ base_bytes,
                                                         uint32_t* __restrict__ base_cnt, uint64_t* __restrict__ totals)
{
	constexpr uint32_t kPer = 4, kStep = 64 * kPer;
	const uint32_t lane = threadIdx.x;
	uint64_t run_b = 0, run_c = 0, bad = 0;
	uint64_t nb[kPer];
	uint32_t nc[kPer], nd[kPer];
	auto load = [&](uint32_t j0) {
#pragma unroll
		for (uint32_t u = 0; u < kPer; ++u)
		{
			const uint32_t j = j0 + lane * kPer + u;
			nb[u] = j < g ? bbytes[j] : 0ull;
			nc[u] = j < g ? bcnt[j] : 0u;
			nd[u] = j < g ? bbad[j] : 0u;
		}
	};
	load(0);
	for (uint32_t j0 = 0; j0 < g; j0 += kStep)
	{
		uint64_t b[kPer], c[kPer], tb = 0, tc = 0;
#pragma unroll
		for (uint32_t u = 0; u < kPer; ++u)
		{
			b[u] = nb[u];
			c[u] = nc[u];
			tb += b[u];
			tc += c[u];
			bad += nd[u];
		}
		if (j0 + kStep < g)
			load(j0 + kStep);
		const uint64_t ib = wave_scan_incl(tb, lane), ic = wave_scan_incl(tc, lane);
		uint64_t eb = run_b + ib - tb, ec = run_c + ic - tc;  // exclusive, at the lane's first block
#pragma unroll
		for (uint32_t u = 0; u < kPer; ++u)
		{
			const uint32_t j = j0 + lane * kPer + u;
			if (j < g)
			{
				base_bytes[j] = eb;
				base_cnt[j] = (uint32_t)ec;  // < the selected packets <= n
			}
			eb += b[u];
			ec += c[u];
		}
		run_b += __shfl(ib, 63);
		run_c += __shfl(ic, 63);
	}
	bad = wave_sum(bad);
	if (lane == 0)
	{
		totals[PCPPX_SEL_SELECTED_PACKETS] = run_c;
		totals[PCPPX_SEL_SELECTED_BYTES] = run_b;
		totals[PCPPX_SEL_WRITTEN_PACKETS] = run_c;
		totals[PCPPX_SEL_WRITTEN_BYTES] = run_b;
		totals[PCPPX_SEL_BAD_DESC] = bad;
		totals[5] = totals[6] = totals[7] = 0;
	}
}

// the packet that holds position lo (qS <= lo < qE) of a tile's span: the last k < nw with dq[k] <= lo (dq ascending,
// dq[0] = qS; zero-length packets ahead of it are passed over). Branch-free: a probe past the last packet reads the
// span's end dq[nw] = qE > lo and is not taken.
__device__ __forceinline__ uint32_t find_packet(const uint64_t* dq, uint32_t nw, uint64_t lo)
{
	uint32_t k = 0;
#pragma unroll
	for (uint32_t step = 32; step != 0; step >>= 1)
	{
		const uint32_t probe = k + step < nw ? k + step : nw;
		k = dq[probe] <= lo ? probe : k;
	}
	return k;
}

// bits [0, 8x) of a 16-byte mask, as its low and high 64 bits (x = 0 .. 16 bytes)
__device__ __forceinline__ void bytes_below(uint32_t x, uint64_t& lo, uint64_t& hi)
{
	lo = x >= 8 ? ~0ull : (1ull << (8 * x)) - 1;
	hi = x <= 8 ? 0ull : (x >= 16 ? ~0ull : (1ull << (8 * (x - 8))) - 1);
}

// the piece [d, d + len) of a chunk, taken from the aligned source granules ga:gb, where ga holds the piece's first
// byte at byte `so` (gb is read only when the piece runs on into it): chunk byte d + t = source byte so + t of ga:gb;
// when d > so the piece lies in ga alone, shifted up. ORed into the chunk's bytes v0:v1.
__device__ __forceinline__ void place_piece(uint4 ga, uint4 gb, uint32_t so, uint32_t d, uint32_t len, uint64_t& v0,
                                            uint64_t& v1)
{
	const uint4 zero = make_uint4(0, 0, 0, 0);
	const bool up = d > so;
	const uint4 r = funnel16(up ? zero : ga, up ? ga : gb, (so - d) & 15);
	uint64_t l0, h0, l1, h1;
	bytes_below(d, l0, h0);
	bytes_below(d + len, l1, h1);
	v0 |= ((uint64_t)r.x | (uint64_t)r.y << 32) & l1 & ~l0;
	v1 |= ((uint64_t)r.z | (uint64_t)r.w << 32) & h1 & ~h0;
}

// Finish a chunk that is not one whole piece -- it straddles packets, or it is the span's partial first / last chunk
// (shared with the neighbouring tile's wave): v0:v1 hold its first piece, [lo, a) of packet k; the pieces of the
// packets behind it are gathered one by one (the one or two aligned source granules that hold the piece, shifted to
// its place). Only the bytes owned, [lo, hi), are stored: one 16-B store when that is the whole chunk, else byte
// stores. sa[k]: packet k's source position, shifted like dq so that position % 16 = address % 16.
__device__ __forceinline__ void finish_chunk(const uint64_t* dq, const uint64_t* sa, uint64_t cs, uint64_t lo,
                                             uint64_t hi, uint64_t a, uint32_t k, uint64_t v0, uint64_t v1,
                                             const uint8_t* sbase, uint8_t* dbase)
{
	while (a < hi)
	{
		uint64_t nxt = dq[k + 1];
		while (nxt <= a)  // the packet's end, then zero-length packets; a < hi <= dq[nw]: ends with k < nw
		{
			++k;
			nxt = dq[k + 1];
		}
		const uint64_t b = nxt < hi ? nxt : hi;  // the piece [a, b) belongs to packet k
		const uint64_t s = sa[k] + (a - dq[k]);
		const uint32_t len = (uint32_t)(b - a), so = (uint32_t)(s & 15);
		const uint4* g = reinterpret_cast<const uint4*>(sbase + (s & ~15ull));
		const uint4 ga = g[0];
		const uint4 gb = g[so + len > 16 ? 1 : 0];
		place_piece(ga, gb, so, (uint32_t)(a - cs), len, v0, v1);
		a = b;
	}
	if (lo == cs && hi == cs + 16)
		*reinterpret_cast<uint4*>(dbase + cs) =
		    make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1, (uint32_t)(v1 >> 32));
	else
	{
#pragma unroll
		for (uint32_t j = 0; j < 16; ++j)
			if (cs + j >= lo && cs + j < hi)
				dbase[cs + j] = (uint8_t)(j < 8 ? v0 >> (8 * j) : v1 >> (8 * (j - 8)));
	}
}

template <typename T>
__device__ __forceinline__ T pick(const T (&v)[kSelUnroll], uint32_t x)
{
	static_assert(kSelUnroll == 4, "pick selects among four");
	return x == 0 ? v[0] : x == 1 ? v[1] : x == 2 ? v[2] : v[3];
}

__global__ __launch_bounds__(kSelThreads) void select_copy_kernel(SelIn p, SelOut o,
                                                                  const uint64_t* __restrict__ base_bytes,
                                                                  const uint32_t* __restrict__ base_cnt)
{
	// per wave, for the tile it is gathering: the written packets' destination positions (shifted so that
	// position % 16 = address % 16), one more entry for the span's end, and each packet's source position, shifted alike
	__shared__ uint64_t s_dq[kSelWaves][65];
	__shared__ uint64_t s_src[kSelWaves][64];
	__shared__ uint64_t s_tb[kSelTiles];  // the tiles' selected bytes / packets
	__shared__ uint32_t s_tc[kSelTiles];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
	for (uint32_t u = 0; u < kSelTilesPerWave; ++u)
	{
		bool sel, bad;
		uint32_t len;
		uint64_t off;
		classify(p, tile_first(kSelectBlockPk, w * kSelTilesPerWave + u) + lane, sel, bad, len, off);
		const uint64_t b = wave_sum(len);
		const uint32_t c = __popcll(__ballot(sel));
		if (lane == 0)
		{
			s_tb[w * kSelTilesPerWave + u] = b;
			s_tc[w * kSelTilesPerWave + u] = c;
		}
	}
	__syncthreads();
	// the wave's first tile starts behind the blocks before this one and the block's tiles before it
	uint64_t tile_pos = base_bytes[blockIdx.x], tile_rank = base_cnt[blockIdx.x];
	for (uint32_t t = 0; t < w * kSelTilesPerWave; ++t)
	{
		tile_pos += s_tb[t];
		tile_rank += s_tc[t];
	}
	const bool copy = o.data != nullptr;
	const auto [dbase, dal] = align16(o.data);  // position q (= byte position + dal) lives at dbase + q
	const auto [sbase, sal] = align16(p.data);  // the same for source positions (= batch offset + sal)
	uint64_t* const dq = s_dq[w];
	uint64_t* const sa = s_src[w];

#pragma unroll 1
	for (uint32_t u = 0; u < kSelTilesPerWave; ++u)
	{
		const uint32_t t = w * kSelTilesPerWave + u;
		const uint64_t i = tile_first(kSelectBlockPk, t) + lane;
		bool sel, bad;
		uint32_t len;
		uint64_t off;
		classify(p, i, sel, bad, len, off);  // the descriptors again (cache hits): no per-tile state held in registers
		const uint64_t bal = __ballot(sel);
		const uint32_t rank = __popcll(bal & ((1ull << lane) - 1));  // among the tile's selected packets
		const uint64_t pos = tile_pos + wave_scan_incl(len, lane) - len;
		const uint64_t r = tile_rank + rank;
		tile_pos += s_tb[t];
		tile_rank += s_tc[t];
		// the written packets are a prefix of the selected ones: both conditions are monotone in source order
		const bool fits = r < o.max_packets && (!copy || pos + len <= o.data_cap);
		const bool wr = sel && fits;
		if (wr)
		{
			o.offsets[r] = pos;
			o.caplens[r] = len;
			if (o.index != nullptr)
				o.index[r] = (uint32_t)i;
		}
		// the first selected packet that is not written (its predecessor, ending at pos, was): it ends the output
		if (sel && !fits && (r == 0 || (r - 1 < o.max_packets && (!copy || pos <= o.data_cap))))
		{
			o.totals[PCPPX_SEL_WRITTEN_PACKETS] = r;
			o.totals[PCPPX_SEL_WRITTEN_BYTES] = pos;
		}
		if (!copy)  // index-only (uniform over the grid)
			continue;
		const uint32_t nw = __popcll(__ballot(wr));  // the tile's written packets: ranks 0 .. nw-1
		if (nw == 0)
			continue;
		// the wave's own LDS rows: its LDS accesses complete in program order, so a wave-level fence (no block barrier:
		// the waves' tiles differ) orders these stores behind the previous tile's loads and ahead of this tile's
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		if (wr)
		{
			dq[rank] = pos + dal;
			sa[rank] = off + sal;
			if (rank == nw - 1)
				dq[nw] = pos + len + dal;
		}
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		const uint64_t qS = dq[0], qE = dq[nw];
		if (qE == qS)  // zero-length packets only
			continue;
		const uint64_t m_last = (qE - 1) >> 4;
		for (uint64_t m0 = (qS >> 4) + lane; m0 <= m_last; m0 += 64 * kSelUnroll)
		{
			// kSelUnroll chunks per lane, 64 chunks apart (the wave's stores stay contiguous). Each chunk's first piece:
			// the packet that owns its first owned byte, up to that packet's end or the chunk's -- almost always the
			// whole chunk. Its two aligned source granules (the second one only if the piece runs on into it, else the
			// first one again) are loaded unconditionally, so every chunk's loads are in flight together; a chunk past
			// the span's end loads the last chunk's again. A whole-chunk piece is funnel-shifted into one 16-B store.
			uint64_t s[kSelUnroll], v0[kSelUnroll], v1[kSelUnroll];
			uint32_t kx[kSelUnroll], len1[kSelUnroll];
			uint32_t live = 0, more = 0;
#pragma unroll
			for (uint32_t x = 0; x < kSelUnroll; ++x)
			{
				live |= (m0 + 64 * x <= m_last ? 1u : 0u) << x;
				const uint64_t cs = ((live >> x) & 1 ? m0 + 64 * x : m_last) << 4;
				const uint64_t lo = cs > qS ? cs : qS, hi = cs + 16 < qE ? cs + 16 : qE;
				const uint32_t k = find_packet(dq, nw, lo);
				const uint64_t end = dq[k + 1];
				kx[x] = k;
				v0[x] = v1[x] = 0;
				s[x] = sa[k] + (lo - dq[k]);
				len1[x] = (uint32_t)((end < hi ? end : hi) - lo);
			}
			uint4 a[kSelUnroll], b[kSelUnroll];
#pragma unroll
			for (uint32_t x = 0; x < kSelUnroll; ++x)
			{
				const uint4* g = reinterpret_cast<const uint4*>(sbase + (s[x] & ~15ull));
				a[x] = g[0];
				b[x] = g[(uint32_t)(s[x] & 15) + len1[x] > 16 ? 1 : 0];
			}
#pragma unroll
			for (uint32_t x = 0; x < kSelUnroll; ++x)
			{
				const uint64_t cs = (m0 + 64 * x) << 4;
				const uint32_t d = cs < qS ? (uint32_t)(qS - cs) : 0u;
				if (((live >> x) & 1) && len1[x] == 16)
					*reinterpret_cast<uint4*>(dbase + cs) = funnel16(a[x], b[x], (uint32_t)(s[x] & 15));
				else if ((live >> x) & 1)
				{
					place_piece(a[x], b[x], (uint32_t)(s[x] & 15), d, len1[x], v0[x], v1[x]);
					more |= 1u << x;
				}
			}
			// the other chunks: each lane finishes its own (rarely more than one), whichever of its chunks they are
			while (more != 0)
			{
				const uint32_t x = __ffs(more) - 1;
				more &= more - 1;
				const uint64_t cs = (m0 + 64 * x) << 4;
				const uint64_t lo = cs > qS ? cs : qS, hi = cs + 16 < qE ? cs + 16 : qE;
				finish_chunk(dq, sa, cs, lo, hi, lo + pick(len1, x), pick(kx, x), pick(v0, x), pick(v1, x), sbase, dbase);
			}
		}
	}
}
}  // namespace

uint32_t select_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kSelectBlockPk - 1) / kSelectBlockPk);
}

uint64_t select_scratch_bytes(uint32_t n)
{
	return (uint64_t)select_blocks(n) * (8 + 8 + 4 + 4 + 4);
}

int launch_select(const pcppx_batch* b, const pcppx_select_spec* s, const pcppx_selection* out, void* scratch,
                  hipStream_t stream)
{
	const uint32_t g = select_blocks(b->n);
	uint64_t* bbytes = static_cast<uint64_t*>(scratch);
	uint64_t* base_bytes = bbytes + g;
	uint32_t* bcnt = reinterpret_cast<uint32_t*>(base_bytes + g);
	uint32_t* bbad = bcnt + g;
	uint32_t* base_cnt = bbad + g;
	SelIn in{ b->data,
		      b->offsets,
		      b->caplens,
		      b->data_len,
		      b->n,
		      s->keep,
		      static_cast<const uint8_t*>(s->flags),
		      s->flags_stride,
		      s->flags_any,
		      s->invert,
		      s->snaplen };
	SelOut o{ out->data, out->data_cap, out->offsets, out->caplens, out->index, out->max_packets, out->totals };
	hipLaunchKernelGGL(select_count_kernel, dim3(g), dim3(kSelThreads), 0, stream, in, bbytes, bcnt, bbad);
	hipLaunchKernelGGL(select_base_kernel, dim3(1), dim3(64), 0, stream, g, bbytes, bcnt, bbad, base_bytes, base_cnt,
	                   out->totals);
	hipLaunchKernelGGL(select_copy_kernel, dim3(g), dim3(kSelThreads), 0, stream, in, o, base_bytes, base_cnt);
	return check_launch("select", stream);
}
}  // namespace pcppx
