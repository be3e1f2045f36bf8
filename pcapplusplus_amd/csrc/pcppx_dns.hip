// pcppx_dns.hip — pcppx_dns_device: DnsLayer's resource records of the DNS packets of a batch in HBM.
//
// The contract is in include/pcppx.h (dns); the layer rule, the resource walk and the name decode are pcppx_dns.h's,
// which pcppx_dns_ref.cpp compiles for the host. Plain launches in stream order; no block waits on another, no thread
// spins, no atomics. Every grid is sized from n: a block owns kDnsBlockPk source packets and their records.
//   dns_plan_kernel  a thread per source packet, 1024 a block: the disposition from the descriptor and the recorded DNS
//                    layer; a message's thread does the whole walk with the counting sink (its records, its name bytes,
//                    its linked queries plus answers). A 16-byte plan per packet; six 32-bit sums per block.
//   dns_base_kernel  one wave: exclusive prefixes of the blocks' messages, records and name bytes, the totals, the
//                    all-or-nothing verdict
//   dns_emit_kernel  exits on overflow. The block's plans with the exclusive prefixes of their messages, records and
//                    name bytes go to LDS; the disposition per source packet. The block's messages are listed densely
//                    in LDS, and thread h takes message h of the list (full waves where the DNS share is low): the
//                    walk again with the emitting sink (32-byte records as whole structs, name bytes one by one), then
//                    the 40-byte message record.
// A block is 1024 threads (16 waves, a wave per 64-packet tile) so that neither kernel loops around the walk: the
// walk's own loop nest is what the scalar registers have to hold.
// All byte positions are 64-bit. Source bytes are read only inside a recorded DNS layer that lies inside an in-bounds
// packet.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"
#include "pcppx_dns.h"

namespace pcppx
{
namespace
{
using namespace move;
using namespace dns;
constexpr uint32_t kDnThreads = kDnsBlockPk, kDnWaves = kDnThreads / 64;  // a thread per packet, a wave per tile
static_assert(kDnThreads == 1024, "the largest block");
static_assert(kDnsBlockPk <= 65536, "s_list holds 16-bit slots");
// a block's records and name bytes fit 32 bits: 300 records of at most 511 bytes per packet
static_assert((uint64_t)kDnsBlockPk * kMaxResources * 511 < (1ull << 32), "32-bit block sums");
constexpr uint32_t kNone = 0xFF;  // a plan's disp past the batch's end (never stored)
constexpr uint32_t kDnSums = 6;   // messages, records, name bytes, host, bad descriptors, queries + answers

// What the emit kernel needs of a source packet, 16 bytes. All but disp: of a message only.
struct Plan
{
	uint32_t name_bytes;
	uint16_t off, L;  // the layer
	uint16_t n_rr, qa;
	uint8_t adj;
	uint8_t disp;  // PCPPX_DNS_* or kNone
	uint8_t pad[2];
};
static_assert(sizeof(Plan) == 16, "dns_scratch_bytes");

struct DnIn
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
	uint32_t sections;
};

struct DnOut
{
	pcppx_dns_msg* msgs;
	pcppx_dns_rr* rrs;
	uint8_t* names;  // null: no text
	uint64_t names_cap;
	uint8_t* disposition;
	uint32_t max_msgs, max_rrs, spec_msgs;  // spec_msgs: resolved (never 0 with n > 0)
	uint64_t* totals;
};

// Packet i's plan (disp kNone past the batch's end).
__device__ __forceinline__ Plan classify(const DnIn& p, uint64_t i)
{
	Plan pl{};
	pl.disp = kNone;
	if (i >= p.n)
		return pl;
	uint64_t off;
	uint32_t cap;
	pl.disp = PCPPX_DNS_BAD_DESC;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return pl;
	const uint8_t* rec = p.rec0 + i * p.rec_stride;
	const uint32_t flags = *reinterpret_cast<const uint16_t*>(rec + 12), n_layers = rec[14];
	const Layer l = find_layer(cap, p.layers + i * p.ml, n_layers, p.ml, flags);
	pl.disp = (uint8_t)l.disp;
	if (l.disp != PCPPX_DNS_MSG)
		return pl;
	CountSink count;
	const Walk w = walk(p.data + off + l.off, l.L, l.adj, p.sections, count);
	pl.off = (uint16_t)l.off;
	pl.L = (uint16_t)l.L;
	pl.adj = (uint8_t)l.adj;
	pl.n_rr = (uint16_t)w.n_rr;
	pl.qa = (uint16_t)(count_of(w.linked, 0) + count_of(w.linked, 1));
	pl.name_bytes = w.name_bytes;
	return pl;
}

__global__ __launch_bounds__(kDnThreads) void dns_plan_kernel(DnIn p, Plan* __restrict__ plan,
                                                              uint32_t* __restrict__ bsums)
{
	__shared__ uint32_t lc[kDnWaves][kDnSums];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t i = tile_first(kDnsBlockPk, w) + lane;
	const Plan pl = classify(p, i);
	if (pl.disp != kNone)
		plan[i] = pl;
	const bool m = pl.disp == PCPPX_DNS_MSG;
	// the tile's sums: 64 packets of at most 300 records and 300 * 511 bytes
	const uint64_t s01 = wave_sum((m ? 1u : 0u) | ((uint64_t)(m ? pl.n_rr : 0u) << 32));
	const uint64_t s25 = wave_sum((m ? pl.name_bytes : 0u) | ((uint64_t)(m ? pl.qa : 0u) << 32));
	const uint64_t s34 = wave_sum((pl.disp == PCPPX_DNS_HOST ? 1u : 0u) |
	                              ((uint64_t)(pl.disp == PCPPX_DNS_BAD_DESC ? 1u : 0u) << 32));
	if (lane == 0)
	{
		lc[w][0] = (uint32_t)s01;
		lc[w][1] = (uint32_t)(s01 >> 32);
		lc[w][2] = (uint32_t)s25;
		lc[w][3] = (uint32_t)s34;
		lc[w][4] = (uint32_t)(s34 >> 32);
		lc[w][5] = (uint32_t)(s25 >> 32);
	}
	__syncthreads();
	if (threadIdx.x < kDnSums)
	{
		const uint32_t k = threadIdx.x;
		uint32_t sum = 0;
		for (uint32_t x = 0; x < kDnWaves; ++x)
			sum += lc[x][k];
		bsums[(uint64_t)k * gridDim.x + blockIdx.x] = sum;
	}
}

// One wave: the exclusive prefixes of the g blocks' messages, records and name bytes (64 a step, a running carry), the
// totals, the verdict. base: three arrays of g.
__global__ __launch_bounds__(64) void dns_base_kernel(uint32_t g, const uint32_t* __restrict__ bsums,
                                                      uint64_t* __restrict__ base, DnOut o)
{
	const uint32_t lane = threadIdx.x;
	uint64_t run[3] = { 0, 0, 0 }, sums[3] = { 0, 0, 0 };
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
#pragma unroll
		for (uint32_t k = 0; k < 3; ++k)
		{
			const uint64_t v = j < g ? bsums[(uint64_t)k * g + j] : 0u;
			const uint64_t iv = wave_scan_incl(v, lane);
			if (j < g)
				base[(uint64_t)k * g + j] = run[k] + iv - v;
			run[k] += __shfl(iv, 63);
			sums[k] += j < g ? bsums[(uint64_t)(k + 3) * g + j] : 0u;
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < 3; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		o.totals[PCPPX_DNS_MSGS] = run[0];
		o.totals[PCPPX_DNS_RRS] = run[1];
		o.totals[PCPPX_DNS_NAME_BYTES] = run[2];
		o.totals[PCPPX_DNS_HOST_N] = sums[0];
		o.totals[PCPPX_DNS_BAD_DESC_N] = sums[1];
		o.totals[PCPPX_DNS_QA_LINKED] = sums[2];
		o.totals[6] = 0;
		o.totals[PCPPX_DNS_OVERFLOW] = (run[0] > o.max_msgs || run[0] > o.spec_msgs || run[1] > o.max_rrs ||
		                                (o.names != nullptr && run[2] > o.names_cap))
		                                   ? 1
		                                   : 0;
	}
}

__global__ __launch_bounds__(kDnThreads) void dns_emit_kernel(DnIn p, DnOut o, const Plan* __restrict__ plan,
                                                              const uint64_t* __restrict__ base, uint32_t g)
{
	__shared__ uint32_t s_cp[kDnsBlockPk];  // 2 * (the tile's messages before the packet) + (the packet is a message)
	__shared__ uint32_t s_rp[kDnsBlockPk];  // the block's records before the packet's
	__shared__ uint32_t s_bp[kDnsBlockPk];  // and its name bytes
	__shared__ uint32_t s_tc[kDnWaves], s_tr[kDnWaves], s_tb[kDnWaves];
	__shared__ uint32_t s_total;              // the block's messages
	__shared__ uint16_t s_list[kDnsBlockPk];  // the block's messages: their slots, in source order
	if (o.totals[PCPPX_DNS_OVERFLOW] != 0)    // all or nothing: the same word for every block
		return;
	const uint32_t lane = threadIdx.x & 63, tl = threadIdx.x >> 6, slot = threadIdx.x;
	const uint64_t first = tile_first(kDnsBlockPk, 0);
	{
		const uint64_t i = first + slot;
		uint32_t disp = kNone, rr = 0, bytes = 0;
		if (i < p.n)
		{
			const Plan pl = plan[i];
			disp = pl.disp;
			rr = pl.n_rr;
			bytes = pl.name_bytes;
			if (o.disposition != nullptr)
				o.disposition[i] = (uint8_t)disp;
		}
		const uint32_t cnt = disp == PCPPX_DNS_MSG ? 1 : 0;
		// one scan for the first two: the tile's sums fit 7 and 15 bits
		const uint64_t packed = cnt | ((uint64_t)(cnt != 0 ? rr : 0u) << 16);
		const uint64_t ip = wave_scan_incl(packed, lane), ib = wave_scan_incl(cnt != 0 ? bytes : 0u, lane);
		const uint32_t ic = (uint32_t)(ip & 0xFFFF), ir = (uint32_t)(ip >> 16);
		s_cp[slot] = ((ic - cnt) << 1) | cnt;
		s_rp[slot] = ir - (cnt != 0 ? rr : 0u);
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
			s_list[bc + (v >> 1)] = (uint16_t)slot;  // below the block's messages <= kDnsBlockPk
		if (slot == kDnsBlockPk - 1)
			s_total = bc + s_tc[tl];
	}
	__syncthreads();
	const uint32_t h = threadIdx.x;  // message h of the block's list
	if (h >= s_total)
		return;
	const uint64_t msg0 = base[blockIdx.x], rr0 = base[(uint64_t)g + blockIdx.x],
	               pos0 = base[2ull * g + blockIdx.x];
	const uint32_t mine = s_list[h];
	const uint64_t i = first + mine;  // < n: a message
	const Plan pl = plan[i];
	const Layer l{ PCPPX_DNS_MSG, pl.off, pl.L, pl.adj };
	const uint8_t* d = p.data + p.offsets[i] + pl.off;
	const uint64_t first_rr = rr0 + s_rp[mine];  // first_rr + n_rr <= RRS <= max_rrs
	EmitSink sink{ o.rrs + first_rr, o.names, pos0 + s_bp[mine], (uint32_t)(msg0 + h) };
	const Walk wk = walk(d, l.L, l.adj, p.sections, sink);
	put_msg(o.msgs + (msg0 + h), first_rr, (uint32_t)i, l, d, wk);  // msg0 + h < MSGS <= max_msgs
}
}  // namespace

uint32_t dns_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kDnsBlockPk - 1) / kDnsBlockPk);
}

uint64_t dns_scratch_bytes(uint32_t n)
{
	return 48ull * dns_blocks(n) + 16ull * n;
}

int launch_dns(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
               const pcppx_dns_spec* spec, const pcppx_dns_out* out, void* scratch, hipStream_t stream)
{
	const uint32_t g = dns_blocks(b->n);
	// plan[n] | the exclusive prefixes of messages, records, name bytes [g each, 64-bit] | six sums [g each, 32-bit]:
	// 16 n + 48 g bytes
	Plan* plan = static_cast<Plan*>(scratch);
	uint64_t* base = reinterpret_cast<uint64_t*>(plan + b->n);
	uint32_t* bsums = reinterpret_cast<uint32_t*>(base + 3ull * g);
	DnIn in{ b->data, b->offsets, b->caplens, b->data_len, b->n, layers, ml, rec0, rec_stride, spec->sections };
	DnOut o{ out->msgs,     out->rrs,     out->names, out->names_cap,
		     out->disposition, out->max_msgs, out->max_rrs, spec->max_msgs == 0 ? b->n : spec->max_msgs,
		     out->totals };
	hipLaunchKernelGGL(dns_plan_kernel, dim3(g), dim3(kDnThreads), 0, stream, in, plan, bsums);
	hipLaunchKernelGGL(dns_base_kernel, dim3(1), dim3(64), 0, stream, g, bsums, base, o);
	hipLaunchKernelGGL(dns_emit_kernel, dim3(g), dim3(kDnThreads), 0, stream, in, o, plan, base, g);
	return check_launch("dns", stream);
}
}  // namespace pcppx
