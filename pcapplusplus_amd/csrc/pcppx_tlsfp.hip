// pcppx_tlsfp.hip — pcppx_tlsfp_device: JA3 / JA3S fingerprints of the hello packets of a batch in HBM
// (TLSFingerprinting).
//
// The contract is in include/pcppx.h (tlsfp); the walk, the text and the MD5 are pcppx_tlsfp.h's, which
// pcppx_tlsfp_ref.cpp compiles for the host. Plain launches in stream order; no block waits on another, no thread
// spins, no atomics. Every grid is sized from n: a block owns kTlsfpBlockPk source packets and their records.
//   tlsfp_plan_kernel  per block, each wave its four 64-packet tiles, a lane per source packet: the disposition from the
//                      descriptor, the recorded handshake layer and its message headers; a hello's lane walks its lists
//                      once and counts the text's bytes (hellos are rare: the lanes of a wave that found none wait for
//                      the few that did). A 16-byte plan per packet; the block's records and text bytes and four counts.
//   tlsfp_base_kernel  one wave: exclusive prefix of the block sums, the totals, the all-or-nothing verdict
//   tlsfp_emit_kernel  exits on overflow. The block's plans with the exclusive prefixes of their records and text bytes
//                      go to LDS; the disposition per source packet. The block's hellos are listed densely in LDS, and
//                      the block walks that list, a thread per hello: the walk again, every text byte into out->text
//                      (when set) and into the hello's MD5 block, which is a column of an LDS array (word w of thread t
//                      at w * 256 + t); the 40-byte record as five 64-bit stores.
// All byte positions are 64-bit. Source bytes are read only inside a recorded SSL layer that lies inside an in-bounds
// packet.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"
#include "pcppx_tlsfp.h"

namespace pcppx
{
namespace
{
using namespace move;
using namespace tlsfp;
constexpr uint32_t kTfThreads = 256, kTfWaves = kTfThreads / 64;
constexpr uint32_t kTfTilesPerWave = 4, kTfTiles = kTfWaves * kTfTilesPerWave;
static_assert(kTfTiles * 64 == kTlsfpBlockPk, "a block takes kTlsfpBlockPk packets");
static_assert(kTlsfpBlockPk <= 65536, "s_list holds 16-bit slots");
constexpr uint32_t kNone = 0xFF;  // a plan's disp past the batch's end (never stored)
constexpr uint32_t kTfSums = 4;   // client hellos, server hellos, host, bad descriptors

// What the emit kernel needs of a source packet, 16 bytes. msg_off / D / M / text_len: of a hello only.
struct Plan
{
	uint32_t msg_off;
	uint16_t D, M;
	uint32_t text_len;
	uint8_t disp;  // PCPPX_TLSFP_* or kNone
	uint8_t pad[3];
};
static_assert(sizeof(Plan) == 16, "tlsfp_scratch_bytes");

struct TfIn
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
	uint32_t client, server;
};

struct TfOut
{
	pcppx_tlsfp_rec* recs;
	uint8_t* text;  // null: MD5 only
	uint64_t text_cap;
	uint8_t* disposition;
	uint32_t max_recs, max_hellos;  // max_hellos: resolved (never 0 with n > 0)
	uint64_t* totals;
};

__device__ __forceinline__ bool is_hello(uint32_t disp)
{
	return disp == PCPPX_TLSFP_CLIENT || disp == PCPPX_TLSFP_SERVER;
}

// Packet i's plan (disp kNone past the batch's end).
__device__ __forceinline__ Plan classify(const TfIn& p, uint64_t i)
{
	Plan pl{};
	pl.disp = kNone;
	if (i >= p.n)
		return pl;
	uint64_t off;
	uint32_t cap;
	pl.disp = PCPPX_TLSFP_BAD_DESC;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return pl;
	const uint8_t* rec = p.rec0 + i * p.rec_stride;
	const uint32_t flags = *reinterpret_cast<const uint16_t*>(rec + 12), n_layers = rec[14];
	const uint8_t* pk = p.data + off;
	const Hello h = find_hello(pk, cap, p.layers + i * p.ml, n_layers, p.ml, flags, p.client != 0, p.server != 0);
	pl.disp = (uint8_t)h.disp;
	if (!is_hello(h.disp))
		return pl;
	CountSink count;
	hello_text(pk + h.msg_off, h.D, h.M, h.disp, count);
	pl.msg_off = h.msg_off;
	pl.D = (uint16_t)h.D;  // D <= 65530
	pl.M = (uint16_t)h.M;
	pl.text_len = count.len;
	return pl;
}

__global__ __launch_bounds__(kTfThreads) void tlsfp_plan_kernel(TfIn p, Plan* __restrict__ plan,
                                                                uint64_t* __restrict__ bcnt,
                                                                uint64_t* __restrict__ bbytes,
                                                                uint32_t* __restrict__ bsums)
{
	__shared__ uint64_t lb[kTfWaves];
	__shared__ uint32_t lc[kTfWaves][kTfSums];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t b = 0;
	uint32_t s[kTfSums] = { 0, 0, 0, 0 };
#pragma unroll 1
	for (uint32_t u = 0; u < kTfTilesPerWave; ++u)
	{
		const uint64_t i = tile_first(kTlsfpBlockPk, w * kTfTilesPerWave + u) + lane;
		const Plan pl = classify(p, i);
		if (pl.disp != kNone)
			plan[i] = pl;
		b += is_hello(pl.disp) ? pl.text_len : 0u;
		s[0] += __popcll(__ballot(pl.disp == PCPPX_TLSFP_CLIENT));
		s[1] += __popcll(__ballot(pl.disp == PCPPX_TLSFP_SERVER));
		s[2] += __popcll(__ballot(pl.disp == PCPPX_TLSFP_HOST));
		s[3] += __popcll(__ballot(pl.disp == PCPPX_TLSFP_BAD_DESC));
	}
	b = wave_sum(b);
	if (lane == 0)
	{
		lb[w] = b;
		for (uint32_t k = 0; k < kTfSums; ++k)
			lc[w][k] = s[k];
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		uint32_t t[kTfSums];
		for (uint32_t k = 0; k < kTfSums; ++k)
			t[k] = lc[0][k] + lc[1][k] + lc[2][k] + lc[3][k];
		bcnt[blockIdx.x] = t[0] + t[1];
		bbytes[blockIdx.x] = lb[0] + lb[1] + lb[2] + lb[3];
		for (uint32_t k = 0; k < kTfSums; ++k)
			bsums[(uint64_t)k * gridDim.x + blockIdx.x] = t[k];
	}
}

// One wave: the exclusive prefix of the g block sums (64 a step, a running carry), the totals, the verdict.
__global__ __launch_bounds__(64) void tlsfp_base_kernel(uint32_t g, const uint64_t* __restrict__ bcnt,
                                                        const uint64_t* __restrict__ bbytes,
                                                        const uint32_t* __restrict__ bsums,
                                                        uint64_t* __restrict__ base_cnt,
                                                        uint64_t* __restrict__ base_bytes, TfOut o)
{
	const uint32_t lane = threadIdx.x;
	uint64_t run_c = 0, run_b = 0, sums[kTfSums] = { 0, 0, 0, 0 };
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
		const uint64_t c = j < g ? bcnt[j] : 0ull, b = j < g ? bbytes[j] : 0ull;
#pragma unroll
		for (uint32_t k = 0; k < kTfSums; ++k)
			sums[k] += j < g ? bsums[(uint64_t)k * g + j] : 0u;
		const uint64_t ic = wave_scan_incl(c, lane), ib = wave_scan_incl(b, lane);
		if (j < g)
		{
			base_cnt[j] = run_c + ic - c;
			base_bytes[j] = run_b + ib - b;
		}
		run_c += __shfl(ic, 63);
		run_b += __shfl(ib, 63);
	}
#pragma unroll
	for (uint32_t k = 0; k < kTfSums; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		const bool no_room = run_c > o.max_hellos;  // then only CANDIDATES, HOST_N, BAD_DESC_N and OVERFLOW are given
		o.totals[PCPPX_TLSFP_CLIENT_N] = no_room ? 0 : sums[0];
		o.totals[PCPPX_TLSFP_SERVER_N] = no_room ? 0 : sums[1];
		o.totals[PCPPX_TLSFP_TEXT_BYTES] = no_room ? 0 : run_b;
		o.totals[PCPPX_TLSFP_HOST_N] = sums[2];
		o.totals[PCPPX_TLSFP_BAD_DESC_N] = sums[3];
		o.totals[PCPPX_TLSFP_CANDIDATES] = run_c;
		o.totals[6] = 0;
		o.totals[PCPPX_TLSFP_OVERFLOW] =
		    (no_room || run_c > o.max_recs || (o.text != nullptr && run_b > o.text_cap)) ? 1 : 0;
	}
}

__global__ __launch_bounds__(kTfThreads) void tlsfp_emit_kernel(TfIn p, TfOut o, const Plan* __restrict__ plan,
                                                                const uint64_t* __restrict__ base_cnt,
                                                                const uint64_t* __restrict__ base_bytes)
{
	__shared__ uint32_t s_cp[kTlsfpBlockPk];  // 2 * (the tile's hellos before the packet) + (the packet is a hello)
	__shared__ uint32_t s_total;              // the block's hellos
	__shared__ uint64_t s_bp[kTlsfpBlockPk];      // and of their text bytes
	__shared__ uint32_t s_tc[kTfTiles];
	__shared__ uint64_t s_tb[kTfTiles];
	__shared__ uint16_t s_list[kTlsfpBlockPk];  // the block's hellos: their slots, in source order
	__shared__ uint32_t s_md[16 * kTfThreads];  // the threads' MD5 blocks, word-interleaved
	if (o.totals[PCPPX_TLSFP_OVERFLOW] != 0)    // all or nothing: the same word for every block
		return;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t first = tile_first(kTlsfpBlockPk, 0);
#pragma unroll 1
	for (uint32_t u = 0; u < kTfTilesPerWave; ++u)
	{
		const uint32_t tl = w * kTfTilesPerWave + u, slot = tl * 64 + lane;
		const uint64_t i = first + slot;
		uint32_t disp = kNone, len = 0;
		if (i < p.n)
		{
			disp = plan[i].disp;
			len = plan[i].text_len;
			if (o.disposition != nullptr)
				o.disposition[i] = (uint8_t)disp;
		}
		const uint64_t cnt = is_hello(disp) ? 1 : 0, bytes = cnt != 0 ? len : 0u;
		const uint64_t ic = wave_scan_incl(cnt, lane), ib = wave_scan_incl(bytes, lane);
		s_cp[slot] = ((uint32_t)(ic - cnt) << 1) | (uint32_t)cnt;
		s_bp[slot] = ib - bytes;
		if (lane == 63)
		{
			s_tc[tl] = (uint32_t)ic;
			s_tb[tl] = ib;
		}
	}
	__syncthreads();
#pragma unroll 1
	for (uint32_t u = 0; u < kTfTilesPerWave; ++u)
	{
		const uint32_t tl = w * kTfTilesPerWave + u, slot = tl * 64 + lane;
		uint32_t bc = 0;
		uint64_t bb = 0;
		for (uint32_t x = 0; x < tl; ++x)
		{
			bc += s_tc[x];
			bb += s_tb[x];
		}
		const uint32_t v = s_cp[slot];
		s_bp[slot] += bb;
		if ((v & 1) != 0)
			s_list[bc + (v >> 1)] = (uint16_t)slot;  // below the block's hellos <= kTlsfpBlockPk
		if (slot == kTlsfpBlockPk - 1)
			s_total = bc + s_tc[tl];
	}
	__syncthreads();
	const uint32_t total = s_total;
	const uint64_t rank0 = base_cnt[blockIdx.x], pos0 = base_bytes[blockIdx.x];
	for (uint32_t h = threadIdx.x; h < total; h += kTfThreads)
	{
		const uint32_t slot = s_list[h];
		const uint64_t i = first + slot;  // < n: a hello
		const Plan pl = plan[i];
		const uint64_t pos = pos0 + s_bp[slot];
		Md5Sink<kTfThreads> sink(s_md + threadIdx.x, o.text != nullptr ? o.text + pos : nullptr);
		hello_text(p.data + p.offsets[i] + pl.msg_off, pl.D, pl.M, pl.disp, sink);
		uint32_t dg[4];
		sink.finish(dg);
		uint64_t* q = reinterpret_cast<uint64_t*>(o.recs + (rank0 + h));  // rank0 + h < CANDIDATES <= max_recs
		q[0] = dg[0] | ((uint64_t)dg[1] << 32);
		q[1] = dg[2] | ((uint64_t)dg[3] << 32);
		q[2] = pos;
		q[3] = pl.text_len | ((uint64_t)i << 32);
		q[4] = (pl.msg_off & 0xFFFFu) | ((uint64_t)pl.disp << 16);  // the reserved bytes: 0
	}
}
}  // namespace

uint32_t tlsfp_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kTlsfpBlockPk - 1) / kTlsfpBlockPk);
}

uint64_t tlsfp_scratch_bytes(uint32_t n)
{
	return 48ull * tlsfp_blocks(n) + 16ull * n;
}

int launch_tlsfp(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
                 const pcppx_tlsfp_spec* spec, const pcppx_tlsfps* out, void* scratch, hipStream_t stream)
{
	const uint32_t g = tlsfp_blocks(b->n);
	// plan[n] | bcnt, bbytes, base_cnt, base_bytes [g each, 64-bit] | four sums [g each, 32-bit]; 16 n + 48 g bytes
	Plan* plan = static_cast<Plan*>(scratch);
	uint64_t* bcnt = reinterpret_cast<uint64_t*>(plan + b->n);
	uint64_t* bbytes = bcnt + g;
	uint64_t* base_cnt = bbytes + g;
	uint64_t* base_bytes = base_cnt + g;
	uint32_t* bsums = reinterpret_cast<uint32_t*>(base_bytes + g);
	TfIn in{ b->data, b->offsets, b->caplens, b->data_len, b->n,         layers,
		     ml,      rec0,       rec_stride, spec->client, spec->server };
	TfOut o{ out->recs,     out->text, out->text_cap, out->disposition,
		     out->max_recs, spec->max_hellos == 0 ? b->n : spec->max_hellos, out->totals };
	hipLaunchKernelGGL(tlsfp_plan_kernel, dim3(g), dim3(kTfThreads), 0, stream, in, plan, bcnt, bbytes, bsums);
	hipLaunchKernelGGL(tlsfp_base_kernel, dim3(1), dim3(64), 0, stream, g, bcnt, bbytes, bsums, base_cnt, base_bytes, o);
	hipLaunchKernelGGL(tlsfp_emit_kernel, dim3(g), dim3(kTfThreads), 0, stream, in, o, plan, base_cnt, base_bytes);
	return check_launch("tlsfp", stream);
}
}  // namespace pcppx
