// pcppx_ssl.hip — pcppx_ssl_device: the SSL/TLS records, the hellos and the SNI of the SSL packets of a batch in HBM.
//
// The contract is in include/pcppx.h (ssl); the chain rule, the entry walk, the handshake walk and the hello records
// are pcppx_ssl.h's, which pcppx_ssl_ref.cpp compiles for the host. Plain launches in stream order; no block waits on
// another, no thread spins, no atomics. Every grid is sized from n: a block owns kSslBlockPk source packets and their
// records.
//   ssl_plan_kernel  a thread per source packet, 1024 a block: the disposition from the descriptor and the recorded
//                    chain; an SSL packet's thread walks its entries and its handshake messages with the counting sink
//                    (its hello records, its name bytes). A 16-byte plan per packet; ten 32-bit sums per block.
//   ssl_base_kernel  one wave: exclusive prefixes of the blocks' messages, hello records and name bytes, the totals,
//                    the all-or-nothing verdict
//   ssl_emit_kernel  exits on overflow. The block's plans with the exclusive prefixes of their messages, hello records
//                    and name bytes go to LDS; the disposition per source packet. The block's messages are listed
//                    densely in LDS, and thread h takes message h of the list (full waves where the SSL share is low):
//                    the walk again with the emitting sink (32-byte hello records as whole structs, name bytes one by
//                    one), then the 32-byte message record.
// A block is 1024 threads (16 waves, a wave per 64-packet tile) so that neither kernel loops around the walk. The LDS
// arrays are written and scanned by the thread's own slot (32-bit words a lane apart: a 32-lane group covers the 32
// banks once) and the list is read at consecutive positions; only the two prefix reads of a message's thread gather
// (s_hp[mine], s_bp[mine]: one read each, ascending slots, a conflict where two slots of a group lie a multiple of 32
// apart). The walks diverge by packet; the dense list keeps the diverging lanes in as few waves as the block's SSL
// packets need.
// All byte positions are 64-bit. Source bytes are read only inside followed SSL entries and the 4 port bytes of an
// in-bounds packet.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"
#include "pcppx_ssl.h"

namespace pcppx
{
namespace
{
using namespace move;
using namespace ssl;
constexpr uint32_t kSlThreads = kSslBlockPk, kSlWaves = kSlThreads / 64;  // a thread per packet, a wave per tile
static_assert(kSlThreads == 1024, "the largest block");
static_assert(kSslBlockPk <= 65536, "s_list holds 16-bit slots");
// a packet has at most 2 hellos an entry and a name of at most 65535 bytes a hello; a block's sums fit 32 bits
constexpr uint64_t kMaxHellosPk = 2ull * PCPPX_MAX_LAYERS;
static_assert(kMaxHellosPk <= 255, "n_hellos is a byte");
static_assert((uint64_t)kSslBlockPk * kMaxHellosPk * 65535 < (1ull << 32), "32-bit block sums");
constexpr uint32_t kNone = 0xFF;  // a plan's disp past the batch's end (never stored)
// messages, hello records, name bytes, client hellos, server hellos, host, bad, payload bytes, alert / app-data packets
constexpr uint32_t kSlSums = 10;

// What the emit kernel and the sums need of a source packet, 16 bytes. All but disp: of a message only.
struct Plan
{
	uint32_t name_bytes;
	uint16_t payload_len;
	uint8_t n_hellos, n_client;
	uint8_t alert, appdata;  // 0 / 1
	uint8_t disp;            // PCPPX_SSL_* or kNone
	uint8_t pad[5];
};
static_assert(sizeof(Plan) == 16, "ssl_scratch_bytes");

struct SlIn
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
	uint32_t kinds;
};

struct SlOut
{
	pcppx_ssl_msg* msgs;
	pcppx_ssl_hello* hellos;
	uint8_t* names;  // null: positions only
	uint64_t names_cap;
	uint8_t* disposition;
	uint32_t max_msgs, max_hellos, spec_msgs;  // spec_msgs: resolved (never 0 with n > 0)
	uint64_t* totals;
};

// in-bounds packet i (its bytes at off, cap of them) through the walk
template <class Sink>
__device__ __forceinline__ Pkt walk_packet(const SlIn& p, uint64_t i, uint64_t off, uint32_t cap, Sink& sink)
{
	const uint8_t* rec = p.rec0 + i * p.rec_stride;
	const uint32_t flags = *reinterpret_cast<const uint16_t*>(rec + 12), n_layers = rec[14];
	return walk(p.data + off, cap, p.layers + i * p.ml, n_layers, p.ml, flags, p.kinds, sink);
}

// Packet i's plan (disp kNone past the batch's end).
__device__ __forceinline__ Plan classify(const SlIn& p, uint64_t i)
{
	Plan pl{};
	pl.disp = kNone;
	if (i >= p.n)
		return pl;
	uint64_t off;
	uint32_t cap;
	pl.disp = PCPPX_SSL_BAD_DESC;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return pl;
	CountSink count;
	const Pkt w = walk_packet(p, i, off, cap, count);
	pl.disp = (uint8_t)w.disp;
	if (w.disp != PCPPX_SSL_MSG)
		return pl;
	pl.name_bytes = count.name_bytes;
	pl.payload_len = (uint16_t)w.payload_len;
	pl.n_hellos = (uint8_t)count.n_hellos;
	pl.n_client = (uint8_t)count.n_client;
	pl.alert = type_count(w, kAlert) != 0 ? 1 : 0;
	pl.appdata = type_count(w, kAppData) != 0 ? 1 : 0;
	return pl;
}

__global__ __launch_bounds__(kSlThreads) void ssl_plan_kernel(SlIn p, Plan* __restrict__ plan,
                                                              uint32_t* __restrict__ bsums)
{
	__shared__ uint32_t lc[kSlWaves][kSlSums];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t i = tile_first(kSslBlockPk, w) + lane;
	const Plan pl = classify(p, i);
	if (pl.disp != kNone)
		plan[i] = pl;
	const bool m = pl.disp == PCPPX_SSL_MSG;
	// the tile's sums, two to a 64-bit word; the name bytes of 64 packets (up to 2 MB each) take a word of their own
	const uint64_t s01 = wave_sum((m ? 1u : 0u) | ((uint64_t)(m ? pl.n_hellos : 0u) << 32));
	const uint64_t s2 = wave_sum(m ? pl.name_bytes : 0u);
	const uint64_t s37 = wave_sum((m ? pl.n_client : 0u) | ((uint64_t)(m ? pl.payload_len : 0u) << 32));
	const uint64_t s56 = wave_sum((pl.disp == PCPPX_SSL_HOST ? 1u : 0u) |
	                              ((uint64_t)(pl.disp == PCPPX_SSL_BAD_DESC ? 1u : 0u) << 32));
	const uint64_t s89 = wave_sum((m ? pl.alert : 0u) | ((uint64_t)(m ? pl.appdata : 0u) << 32));
	if (lane == 0)
	{
		lc[w][0] = (uint32_t)s01;
		lc[w][1] = (uint32_t)(s01 >> 32);
		lc[w][2] = (uint32_t)s2;
		lc[w][3] = (uint32_t)s37;
		lc[w][4] = (uint32_t)(s01 >> 32) - (uint32_t)s37;  // the server hellos
		lc[w][5] = (uint32_t)s56;
		lc[w][6] = (uint32_t)(s56 >> 32);
		lc[w][7] = (uint32_t)(s37 >> 32);
		lc[w][8] = (uint32_t)s89;
		lc[w][9] = (uint32_t)(s89 >> 32);
	}
	__syncthreads();
	if (threadIdx.x < kSlSums)
	{
		const uint32_t k = threadIdx.x;
		uint32_t sum = 0;
		for (uint32_t x = 0; x < kSlWaves; ++x)
			sum += lc[x][k];
		bsums[(uint64_t)k * gridDim.x + blockIdx.x] = sum;
	}
}

// One wave: the exclusive prefixes of the g blocks' messages, hello records and name bytes (64 a step, a running
// carry), the totals, the verdict. base: three arrays of g.
__global__ __launch_bounds__(64) void ssl_base_kernel(uint32_t g, const uint32_t* __restrict__ bsums,
                                                      uint64_t* __restrict__ base, SlOut o)
{
	const uint32_t lane = threadIdx.x;
	uint64_t run[3] = { 0, 0, 0 }, sums[7] = { 0, 0, 0, 0, 0, 0, 0 };
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
		}
#pragma unroll
		for (uint32_t k = 0; k < 7; ++k)
			sums[k] += j < g ? bsums[(uint64_t)(k + 3) * g + j] : 0u;
	}
#pragma unroll
	for (uint32_t k = 0; k < 7; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		o.totals[PCPPX_SSL_MSGS] = run[0];
		o.totals[PCPPX_SSL_HELLOS] = run[1];
		o.totals[PCPPX_SSL_CLIENT_HELLOS] = sums[0];
		o.totals[PCPPX_SSL_SERVER_HELLOS] = sums[1];
		o.totals[PCPPX_SSL_NAME_BYTES] = run[2];
		o.totals[PCPPX_SSL_HOST_N] = sums[2];
		o.totals[PCPPX_SSL_BAD_DESC_N] = sums[3];
		o.totals[PCPPX_SSL_PAYLOAD_BYTES] = sums[4];
		o.totals[PCPPX_SSL_ALERT_PKTS] = sums[5];
		o.totals[PCPPX_SSL_APPDATA_PKTS] = sums[6];
		o.totals[10] = 0;
		o.totals[PCPPX_SSL_OVERFLOW] = (run[0] > o.max_msgs || run[0] > o.spec_msgs || run[1] > o.max_hellos ||
		                                (o.names != nullptr && run[2] > o.names_cap))
		                                   ? 1
		                                   : 0;
	}
}

__global__ __launch_bounds__(kSlThreads) void ssl_emit_kernel(SlIn p, SlOut o, const Plan* __restrict__ plan,
                                                              const uint64_t* __restrict__ base, uint32_t g)
{
	__shared__ uint32_t s_cp[kSslBlockPk];  // 2 * (the tile's messages before the packet) + (the packet is a message)
	__shared__ uint32_t s_hp[kSslBlockPk];  // the block's hello records before the packet's
	__shared__ uint32_t s_bp[kSslBlockPk];  // and its name bytes
	__shared__ uint32_t s_tc[kSlWaves], s_th[kSlWaves], s_tb[kSlWaves];
	__shared__ uint32_t s_total;              // the block's messages
	__shared__ uint16_t s_list[kSslBlockPk];  // the block's messages: their slots, in source order
	if (o.totals[PCPPX_SSL_OVERFLOW] != 0)    // all or nothing: the same word for every block
		return;
	const uint32_t lane = threadIdx.x & 63, tl = threadIdx.x >> 6, slot = threadIdx.x;
	const uint64_t first = tile_first(kSslBlockPk, 0);
	{
		const uint64_t i = first + slot;
		uint32_t disp = kNone, hel = 0, bytes = 0;
		if (i < p.n)
		{
			const Plan pl = plan[i];
			disp = pl.disp;
			hel = pl.n_hellos;
			bytes = pl.name_bytes;
			if (o.disposition != nullptr)
				o.disposition[i] = (uint8_t)disp;
		}
		const uint32_t cnt = disp == PCPPX_SSL_MSG ? 1 : 0;
		// one scan for the first two: the tile's sums fit 7 and 11 bits
		const uint64_t packed = cnt | ((uint64_t)(cnt != 0 ? hel : 0u) << 16);
		const uint64_t ip = wave_scan_incl(packed, lane), ib = wave_scan_incl(cnt != 0 ? bytes : 0u, lane);
		const uint32_t ic = (uint32_t)(ip & 0xFFFF), ih = (uint32_t)(ip >> 16);
		s_cp[slot] = ((ic - cnt) << 1) | cnt;
		s_hp[slot] = ih - (cnt != 0 ? hel : 0u);
		s_bp[slot] = (uint32_t)ib - (cnt != 0 ? bytes : 0u);
		if (lane == 63)
		{
			s_tc[tl] = ic;
			s_th[tl] = ih;
			s_tb[tl] = (uint32_t)ib;
		}
	}
	__syncthreads();
	{
		uint32_t bc = 0, bh = 0, bb = 0;
		for (uint32_t x = 0; x < tl; ++x)
		{
			bc += s_tc[x];
			bh += s_th[x];
			bb += s_tb[x];
		}
		const uint32_t v = s_cp[slot];
		s_hp[slot] += bh;
		s_bp[slot] += bb;
		if ((v & 1) != 0)
			s_list[bc + (v >> 1)] = (uint16_t)slot;  // below the block's messages <= kSslBlockPk
		if (slot == kSslBlockPk - 1)
			s_total = bc + s_tc[tl];
	}
	__syncthreads();
	const uint32_t h = threadIdx.x;  // message h of the block's list
	if (h >= s_total)
		return;
	const uint64_t msg0 = base[blockIdx.x], hel0 = base[(uint64_t)g + blockIdx.x], pos0 = base[2ull * g + blockIdx.x];
	const uint32_t mine = s_list[h];
	const uint64_t i = first + mine;  // < n: a message, so in bounds
	const uint64_t first_hello = hel0 + s_hp[mine];  // first_hello + n_hellos <= HELLOS <= max_hellos
	EmitSink sink{ o.hellos + first_hello, o.names, pos0 + s_bp[mine], (uint32_t)(msg0 + h) };
	const Pkt wk = walk_packet(p, i, p.offsets[i], p.caplens[i], sink);
	put_msg(o.msgs + (msg0 + h), first_hello, (uint32_t)i, wk, sink.n_hellos, sink.name_bytes);  // msg0 + h < MSGS
}
}  // namespace

uint32_t ssl_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kSslBlockPk - 1) / kSslBlockPk);
}

uint64_t ssl_scratch_bytes(uint32_t n)
{
	return 64ull * ssl_blocks(n) + 16ull * n;
}

int launch_ssl(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
               const pcppx_ssl_spec* spec, const pcppx_ssl_out* out, void* scratch, hipStream_t stream)
{
	const uint32_t g = ssl_blocks(b->n);
	// plan[n] | the exclusive prefixes of messages, hello records, name bytes [g each, 64-bit] | ten sums [g each,
	// 32-bit]: 16 n + 64 g bytes
	Plan* plan = static_cast<Plan*>(scratch);
	uint64_t* base = reinterpret_cast<uint64_t*>(plan + b->n);
	uint32_t* bsums = reinterpret_cast<uint32_t*>(base + 3ull * g);
	SlIn in{ b->data, b->offsets, b->caplens, b->data_len, b->n, layers, ml, rec0, rec_stride, spec->kinds };
	SlOut o{ out->msgs,        out->hellos,   out->names,      out->names_cap,
		     out->disposition, out->max_msgs, out->max_hellos, spec->max_msgs == 0 ? b->n : spec->max_msgs,
		     out->totals };
	hipLaunchKernelGGL(ssl_plan_kernel, dim3(g), dim3(kSlThreads), 0, stream, in, plan, bsums);
	hipLaunchKernelGGL(ssl_base_kernel, dim3(1), dim3(64), 0, stream, g, bsums, base, o);
	hipLaunchKernelGGL(ssl_emit_kernel, dim3(g), dim3(kSlThreads), 0, stream, in, o, plan, base, g);
	return check_launch("ssl", stream);
}
}  // namespace pcppx
