// pcppx_dhcp.hip — pcppx_dhcp_device: the DHCP and DHCPv6 messages and their options of a batch in HBM.
//
// The contract is in include/pcppx.h (dhcp); the dispatch, the two option walks and the typed values are
// pcppx_dhcp.h's, which pcppx_dhcp_ref.cpp compiles for the host. Plain launches in stream order; no block waits on
// another, no thread spins, no atomics. Every grid is sized from n: a block owns kDhcpBlockPk source packets and their
// records. The shape is pcppx_sip.hip's:
//   dhcp_plan_kernel  a thread per source packet, 1024 a block: the disposition from the descriptor, the recorded UDP
//                     entry and its four port bytes (rules 1-7); a message's thread does the whole walk with the
//                     counting sink (its option records, its value bytes, its linked options). A 16-byte plan per
//                     packet; nine 32-bit sums per block.
//   dhcp_base_kernel  one wave: exclusive prefixes of the blocks' messages, records and value bytes, the totals, the
//                     all-or-nothing verdict
//   dhcp_emit_kernel  exits on overflow. The block's plans with the exclusive prefixes of their messages, records and
//                     value bytes go to LDS; the disposition per source packet. The block's messages are listed
//                     densely in LDS, and thread h takes message h of the list (full waves where the DHCP share is
//                     low): the walk again with the emitting sink, then the 80-byte message record.
// A block is 1024 threads (16 waves, a wave per 64-packet tile) so that neither kernel loops around the walk. The spec
// (72 bytes) is copied to LDS first, so that the code lookups index LDS and not a register array.
// All byte positions are 64-bit. Source bytes are read only inside the UDP payload of an in-bounds packet, plus the UDP
// header's four port bytes. The walk is a chain of dependent one- and two-byte loads from HBM, a step per option: that
// latency, not bandwidth, is a message's cost, and it is linear in the payload's length.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"
#include "pcppx_dhcp.h"

namespace pcppx
{
namespace
{
using namespace move;
using namespace dhcp;
constexpr uint32_t kDhThreads = kDhcpBlockPk, kDhWaves = kDhThreads / 64;  // a thread per packet, a wave per tile
static_assert(kDhThreads == 1024, "the largest block");
static_assert(kDhcpBlockPk <= 65536, "s_list holds 16-bit slots");
// a block's records and value bytes fit 32 bits: each at most 65535 per packet
static_assert((uint64_t)kDhcpBlockPk * 65535 < (1ull << 32), "32-bit block sums");
constexpr uint32_t kNone = 0xFF;  // a plan's disp past the batch's end (never stored)
// messages, records, value bytes, DHCPv4, DHCPv6, host, bad, linked options, replies
constexpr uint32_t kDhSums = 9, kDhBases = 3;
constexpr uint32_t kSpecWords = sizeof(pcppx_dhcp_spec) / 4;
static_assert(sizeof(pcppx_dhcp_spec) == 72 && sizeof(pcppx_dhcp_option) == 16 && sizeof(pcppx_dhcp_msg) == 80 &&
                  sizeof(pcppx_dhcp_out) == 64,
              "include/pcppx.h");
static_assert(sizeof(pcppx_dhcp_spec) % 4 == 0, "copied to LDS by words");

// What the emit kernel needs of a source packet, 16 bytes. All but disp: of a message only.
struct Plan
{
	uint16_t off, L;  // the layer
	uint16_t n_rec, value_len;
	uint16_t n_options;
	uint8_t family;  // 4 | 6
	uint8_t disp;    // PCPPX_DHCP_* or kNone
	uint8_t reply;
	uint8_t pad[3];
};
static_assert(sizeof(Plan) == 16, "dhcp_scratch_bytes");

struct DhIn
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

struct DhOut
{
	pcppx_dhcp_msg* msgs;
	pcppx_dhcp_option* options;
	uint8_t* values;  // null: no bytes
	uint64_t values_cap;
	uint8_t* disposition;
	uint32_t max_msgs, max_options, spec_msgs;  // spec_msgs: resolved (never 0 with n > 0)
	uint64_t* totals;
};

// the spec from the kernel's arguments to LDS, a word a thread; the caller synchronises
__device__ __forceinline__ void stage_spec(const pcppx_dhcp_spec& spec, uint32_t* s_spec)
{
	if (threadIdx.x < kSpecWords)
		s_spec[threadIdx.x] = reinterpret_cast<const uint32_t*>(&spec)[threadIdx.x];
}

// Packet i's plan (disp kNone past the batch's end).
__device__ __forceinline__ Plan classify(const DhIn& p, const pcppx_dhcp_spec* spec, uint64_t i)
{
	Plan pl{};
	pl.disp = kNone;
	if (i >= p.n)
		return pl;
	uint64_t off;
	uint32_t cap;
	pl.disp = PCPPX_DHCP_BAD_DESC;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return pl;
	const uint8_t* rec = p.rec0 + i * p.rec_stride;
	const uint32_t flags = *reinterpret_cast<const uint16_t*>(rec + 12), n_layers = rec[14];
	const Layer l = find_layer(p.data + off, cap, p.layers + i * p.ml, n_layers, p.ml, flags, spec->families);
	pl.disp = (uint8_t)l.disp;
	if (l.disp != PCPPX_DHCP_MSG)
		return pl;
	const uint8_t* d = p.data + off + l.off;
	CountSink count;
	const Walk w = walk(d, l.L, l.family, spec, count);
	pl.off = (uint16_t)l.off;
	pl.L = (uint16_t)l.L;
	pl.family = (uint8_t)l.family;
	pl.reply = is_reply(d, l.family) ? 1 : 0;
	pl.n_rec = (uint16_t)w.n_rec;
	pl.value_len = (uint16_t)w.value_len;
	pl.n_options = (uint16_t)w.n_options;
	return pl;
}

__global__ __launch_bounds__(kDhThreads) void dhcp_plan_kernel(DhIn p, pcppx_dhcp_spec spec, Plan* __restrict__ plan,
                                                               uint32_t* __restrict__ bsums)
{
	__shared__ uint32_t lc[kDhWaves][kDhSums];
	__shared__ uint32_t s_spec[kSpecWords];
	stage_spec(spec, s_spec);
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t i = tile_first(kDhcpBlockPk, w) + lane;
	const Plan pl = classify(p, reinterpret_cast<const pcppx_dhcp_spec*>(s_spec), i);
	if (pl.disp != kNone)
		plan[i] = pl;
	const bool m = pl.disp == PCPPX_DHCP_MSG;
	// the tile's sums: 64 packets of at most 65535 each
	const uint64_t s01 = wave_sum((m ? 1u : 0u) | ((uint64_t)(m ? pl.n_rec : 0u) << 32));
	const uint64_t s27 = wave_sum((m ? pl.value_len : 0u) | ((uint64_t)(m ? pl.n_options : 0u) << 32));
	const uint64_t s34 = wave_sum((m && pl.family == 4 ? 1u : 0u) | ((uint64_t)(m && pl.family == 6 ? 1u : 0u) << 32));
	const uint64_t s56 = wave_sum((pl.disp == PCPPX_DHCP_HOST ? 1u : 0u) |
	                              ((uint64_t)(pl.disp == PCPPX_DHCP_BAD_DESC ? 1u : 0u) << 32));
	const uint64_t s8 = wave_sum(m && pl.reply != 0 ? 1u : 0u);
	if (lane == 0)
	{
		lc[w][0] = (uint32_t)s01;
		lc[w][1] = (uint32_t)(s01 >> 32);
		lc[w][2] = (uint32_t)s27;
		lc[w][3] = (uint32_t)s34;
		lc[w][4] = (uint32_t)(s34 >> 32);
		lc[w][5] = (uint32_t)s56;
		lc[w][6] = (uint32_t)(s56 >> 32);
		lc[w][7] = (uint32_t)(s27 >> 32);
		lc[w][8] = (uint32_t)s8;
	}
	__syncthreads();
	if (threadIdx.x < kDhSums)
	{
		const uint32_t k = threadIdx.x;
		uint32_t sum = 0;
		for (uint32_t x = 0; x < kDhWaves; ++x)
			sum += lc[x][k];
		bsums[(uint64_t)k * gridDim.x + blockIdx.x] = sum;
	}
}

// One wave: the exclusive prefixes of the g blocks' messages, records and value bytes (64 a step, a running carry),
// the totals, the verdict. base: three arrays of g.
__global__ __launch_bounds__(64) void dhcp_base_kernel(uint32_t g, const uint32_t* __restrict__ bsums,
                                                       uint64_t* __restrict__ base, DhOut o)
{
	constexpr uint32_t kRest = kDhSums - kDhBases;
	const uint32_t lane = threadIdx.x;
	uint64_t run[kDhBases] = {}, sums[kRest] = {};
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
#pragma unroll
		for (uint32_t k = 0; k < kDhBases; ++k)
		{
			const uint64_t v = j < g ? bsums[(uint64_t)k * g + j] : 0u;
			const uint64_t iv = wave_scan_incl(v, lane);
			if (j < g)
				base[(uint64_t)k * g + j] = run[k] + iv - v;
			run[k] += __shfl(iv, 63);
		}
#pragma unroll
		for (uint32_t k = 0; k < kRest; ++k)
			sums[k] += j < g ? bsums[(uint64_t)(k + kDhBases) * g + j] : 0u;
	}
#pragma unroll
	for (uint32_t k = 0; k < kRest; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		o.totals[PCPPX_DHCP_MSGS] = run[0];
		o.totals[PCPPX_DHCP_V4_N] = sums[0];
		o.totals[PCPPX_DHCP_V6_N] = sums[1];
		o.totals[PCPPX_DHCP_OPTIONS] = run[1];
		o.totals[PCPPX_DHCP_VALUE_BYTES] = run[2];
		o.totals[PCPPX_DHCP_HOST_N] = sums[2];
		o.totals[PCPPX_DHCP_BAD_DESC_N] = sums[3];
		o.totals[PCPPX_DHCP_OPTIONS_LINKED] = sums[4];
		o.totals[PCPPX_DHCP_REPLIES] = sums[5];
		o.totals[PCPPX_DHCP_OVERFLOW] = (run[0] > o.max_msgs || run[0] > o.spec_msgs || run[1] > o.max_options ||
		                                 (o.values != nullptr && run[2] > o.values_cap))
		                                    ? 1
		                                    : 0;
	}
}

__global__ __launch_bounds__(kDhThreads) void dhcp_emit_kernel(DhIn p, pcppx_dhcp_spec spec, DhOut o,
                                                               const Plan* __restrict__ plan,
                                                               const uint64_t* __restrict__ base, uint32_t g)
{
	__shared__ uint32_t s_cp[kDhcpBlockPk];  // 2 * (the tile's messages before the packet) + (the packet is a message)
	__shared__ uint32_t s_rp[kDhcpBlockPk];  // the block's records before the packet's
	__shared__ uint32_t s_bp[kDhcpBlockPk];  // and its value bytes
	__shared__ uint32_t s_tc[kDhWaves], s_tr[kDhWaves], s_tb[kDhWaves];
	__shared__ uint32_t s_total;               // the block's messages
	__shared__ uint16_t s_list[kDhcpBlockPk];  // the block's messages: their slots, in source order
	__shared__ uint32_t s_spec[kSpecWords];
	if (o.totals[PCPPX_DHCP_OVERFLOW] != 0)    // all or nothing: the same word for every block
		return;
	stage_spec(spec, s_spec);
	const uint32_t lane = threadIdx.x & 63, tl = threadIdx.x >> 6, slot = threadIdx.x;
	const uint64_t first = tile_first(kDhcpBlockPk, 0);
	{
		const uint64_t i = first + slot;
		uint32_t disp = kNone, rec = 0, bytes = 0;
		if (i < p.n)
		{
			const Plan pl = plan[i];
			disp = pl.disp;
			rec = pl.n_rec;
			bytes = pl.value_len;
			if (o.disposition != nullptr)
				o.disposition[i] = (uint8_t)disp;
		}
		const uint32_t cnt = disp == PCPPX_DHCP_MSG ? 1 : 0;
		// one scan for two: the tile's sums fit 7 and 22 bits
		const uint64_t packed = cnt | ((uint64_t)(cnt != 0 ? rec : 0u) << 16);
		const uint64_t ip = wave_scan_incl(packed, lane), ib = wave_scan_incl(cnt != 0 ? bytes : 0u, lane);
		const uint32_t ic = (uint32_t)(ip & 0xFF), ir = (uint32_t)(ip >> 16);
		s_cp[slot] = ((ic - cnt) << 1) | cnt;
		s_rp[slot] = ir - (cnt != 0 ? rec : 0u);
		s_bp[slot] = (uint32_t)ib - (cnt != 0 ? bytes : 0u);
		if (lane == 63)
		{
			s_tc[tl] = ic;
			s_tr[tl] = ir;
			s_tb[tl] = (uint32_t)ib;
		}
	}
	__syncthreads();
	{
		uint32_t bc = 0, br = 0, bb = 0;
		for (uint32_t x = 0; x < tl; ++x)
		{
			bc += s_tc[x];
			br += s_tr[x];
			bb += s_tb[x];
		}
		const uint32_t v = s_cp[slot];
		s_rp[slot] += br;
		s_bp[slot] += bb;
		if ((v & 1) != 0)
			s_list[bc + (v >> 1)] = (uint16_t)slot;  // below the block's messages <= kDhcpBlockPk
		if (slot == kDhcpBlockPk - 1)
			s_total = bc + s_tc[tl];
	}
	__syncthreads();
	const uint32_t h = threadIdx.x;  // message h of the block's list
	if (h >= s_total)
		return;
	const uint64_t msg0 = base[blockIdx.x], rec0 = base[(uint64_t)g + blockIdx.x], pos0 = base[2ull * g + blockIdx.x];
	const uint32_t mine = s_list[h];
	const uint64_t i = first + mine;  // < n: a message
	const Plan pl = plan[i];
	const Layer l{ PCPPX_DHCP_MSG, pl.off, pl.L, pl.family };
	const uint8_t* d = p.data + p.offsets[i] + pl.off;
	const uint64_t first_option = rec0 + s_rp[mine];  // first_option + n_rec <= OPTIONS <= max_options
	const uint64_t value_pos = pos0 + s_bp[mine];     // value_pos + value_len <= VALUE_BYTES <= values_cap
	EmitSink sink{ o.options + first_option, o.values, value_pos, (uint32_t)(msg0 + h) };
	const Walk wk = walk(d, l.L, l.family, reinterpret_cast<const pcppx_dhcp_spec*>(s_spec), sink);
	put_msg(o.msgs + (msg0 + h), first_option, value_pos, (uint32_t)i, d, l, wk);  // msg0 + h < MSGS <= max_msgs
}
}  // namespace

uint32_t dhcp_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kDhcpBlockPk - 1) / kDhcpBlockPk);
}

uint64_t dhcp_scratch_bytes(uint32_t n)
{
	return 60ull * dhcp_blocks(n) + 16ull * n;
}

int launch_dhcp(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
                const pcppx_dhcp_spec* spec, const pcppx_dhcp_out* out, void* scratch, hipStream_t stream)
{
	const uint32_t g = dhcp_blocks(b->n);
	// plan[n] | the exclusive prefixes of messages, records, value bytes [g each, 64-bit] | nine sums [g each, 32-bit]:
	// 16 n + 60 g bytes
	Plan* plan = static_cast<Plan*>(scratch);
	uint64_t* base = reinterpret_cast<uint64_t*>(plan + b->n);
	uint32_t* bsums = reinterpret_cast<uint32_t*>(base + (uint64_t)kDhBases * g);
	DhIn in{ b->data, b->offsets, b->caplens, b->data_len, b->n, layers, ml, rec0, rec_stride };
	DhOut o{ out->msgs,     out->options,     out->values, out->values_cap,
		     out->disposition, out->max_msgs, out->max_options, spec->max_msgs == 0 ? b->n : spec->max_msgs,
		     out->totals };
	hipLaunchKernelGGL(dhcp_plan_kernel, dim3(g), dim3(kDhThreads), 0, stream, in, *spec, plan, bsums);
	hipLaunchKernelGGL(dhcp_base_kernel, dim3(1), dim3(64), 0, stream, g, bsums, base, o);
	hipLaunchKernelGGL(dhcp_emit_kernel, dim3(g), dim3(kDhThreads), 0, stream, in, *spec, o, plan, base, g);
	return check_launch("dhcp", stream);
}
}  // namespace pcppx
