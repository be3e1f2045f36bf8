// pcppx_frag.hip — pcppx_frag_device / pcppx_frag6_device: split the IPv4 (and IPv6) packets of a batch in HBM into
// fragments (IPFragUtil).
//
// The contract is in include/pcppx.h (frag, frag6). Every kernel but the base one is a template over k6: <false> is
// pcppx_frag_device's and pcppx_frag6_device's with families = V4 (no IPv6 layer is looked for), <true> takes the
// IPv6 packets too: the plan kernel refines classify()'s verdict (classify_families; classify() itself stays as it
// was, so that <false> compiles to the instructions it always did), takes the first IPv6 layer of a packet without an
// IPv4 one, walks its extension chain (at most PCPPX_FRAG6_MAX_EXT steps) and keeps hdr and the place of the last
// next-header byte in the plan's
// spare words; an IPv6 fragment is head span, an 8-byte gap, piece span, and the patch kernel alone writes the gap (the
// fragment header), the next-header byte and the payload length. No span's store touches a gap byte: copy_spans writes
// exactly [q, q + len) of each span (whole chunks only inside it, its head and tail byte-exact), and the two spans of a
// fragment end and begin at the gap's two ends. Plain launches in stream order; no block waits on another, no thread
// spins, no atomics. One source packet puts out up to 8,190 packets, and how many is known only on the device, so
// every grid is sized from n: a block owns kFragBlockPk source packets and all of their output packets.
//   frag_plan_kernel   per block, each wave its four 64-packet tiles, a lane per source packet: the disposition from the
//                      descriptor, the keep column, the recorded IPv4 layer and the header's fragment word; for a SPLIT
//                      packet the 16-bit sum of its header without the three words every fragment rewrites. A 12-byte
//                      plan per packet; the block's output packets and bytes and five counts.
//   frag_base_kernel   one wave: exclusive prefix of the block sums, the totals, the all-or-nothing verdict
//   frag_emit_kernel   exits on overflow. The block's plans, with the exclusive prefixes of their output counts and
//                      bytes, go to LDS; counts / disposition per source packet. Then the block walks its output
//                      packets, each wave 64 at a time, a lane per OUTPUT packet: the lane finds its source packet by
//                      a ten-step search in the count prefix, writes the descriptor and the per-output columns, and the
//                      wave copies the 64 packets' headers and then their pieces (the tile copy of pcppx_steer.hip and
//                      pcppx_defrag.hip: the spans' whole destination 16-B chunks as one flattened list over the lanes,
//                      each span's head and tail its own). A datagram's fragments are spread over lanes and waves
//                      like any other output packets: an uneven tile costs what its output costs.
//   frag_patch_kernel  only with out->data; a thread per output packet, found as in the emit kernel: total length,
//                      fragment word and header checksum of every fragment, from the plan alone (no read of what the
//                      emit kernel stored). A launch of its own: the six bytes lie in spans other lanes copy.
// All byte positions are 64-bit. Source bytes are read only through aligned 16-B granules that hold a byte of a packet
// that is emitted, or as single bytes of the IPv4 header of an in-bounds, selected packet.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"

namespace pcppx
{
namespace
{
using namespace move;
constexpr uint32_t kFrThreads = 256, kFrWaves = kFrThreads / 64;
constexpr uint32_t kFrTilesPerWave = 4, kFrTiles = kFrWaves * kFrTilesPerWave;
static_assert(kFrTiles * 64 == kFragBlockPk, "a block takes kFragBlockPk packets");
constexpr uint32_t kFrUnroll = 4;   // 16-B chunks a lane has in flight in the copy loop
constexpr uint32_t kProtoIPv4 = 2;  // pcpp::IPv4
constexpr uint32_t kProtoIPv6 = 3;  // pcpp::IPv6
constexpr uint32_t kProtoEth = 1, kProtoVlan = 9, kProtoSll = 19;  // pcpp::Ethernet, VLAN, SLL
constexpr uint32_t kV6Fixed = 40, kV6FragHdr = 8;
constexpr uint32_t kPlanV6 = 1u << 31;  // Plan::sum of an IPv6 packet
constexpr uint32_t kNone = 0xFF;    // a plan's disp past the batch's end (never stored)
constexpr uint32_t kFrSums = 5;     // split packets, fragments, copied, under size, bad descriptors

// What the later kernels need of a source packet, 12 bytes. ip_off / pay / hdr / sum: of a SPLIT packet only.
struct Plan
{
	// IPv4: the header's 16-bit words but total length, fragment word and checksum, added up (< 2^21).
	// IPv6 (<true> only): kPlanV6 | the offset of the last next-header byte from ip_off (< 2^16)
	uint32_t sum;
	uint16_t ip_off, pay;
	uint8_t hdr, disp;  // hdr: IPv4's; disp: PCPPX_FRAG_* or kNone
	uint16_t hdr6;      // IPv6's hdr: the fixed header and the extensions (0 for IPv4)
};
static_assert(sizeof(Plan) == 12, "frag_scratch_bytes");

struct FrIn
{
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	uint64_t data_len;
	uint32_t n;
	const pcppx_layer* layers;
	uint32_t ml;
	const uint8_t* n_layers;
	uint32_t nl_stride;
	const uint8_t* keep;
	uint32_t frag_size, mtu;
	uint32_t copy_rest, honor_df;
};

// the <true> kernels' input: the families asked for (V6 is among them) and the fragment ids
struct FrIn6 : FrIn
{
	uint32_t families, id_base;
	const uint32_t* ids;
};
template <bool k6>
using In = std::conditional_t<k6, FrIn6, FrIn>;

struct FrOut
{
	uint8_t* data;  // null: index-only
	uint64_t data_cap;
	uint64_t* offsets;
	uint32_t* caplens;
	uint32_t* index;
	uint16_t* frag_no;
	uint16_t* counts;
	uint8_t* disposition;
	uint32_t max_packets;
	uint64_t* totals;
};

// the fragment size of a packet with a header of hdr bytes (20..60): >= 8 in both modes
__device__ __forceinline__ uint32_t frag_fs(const FrIn& p, uint32_t hdr)
{
	return p.frag_size != 0 ? p.frag_size : ((p.mtu - hdr) & ~7u);
}

// A SPLIT packet's plan read for either family: the bytes ahead of the payload (head), the gap behind them that the
// patch kernel fills (IPv6's fragment header) and the fragment size (IPv6, mtu mode: mtu >= hdr + 16, so fs >= 8)
template <bool k6>
__device__ __forceinline__ void split_shape(const FrIn& p, const Plan& pl, uint32_t& head, uint32_t& gap, uint32_t& fs)
{
	if constexpr (k6)
	{
		if ((pl.sum & kPlanV6) != 0)
		{
			head = (uint32_t)pl.ip_off + pl.hdr6;
			gap = kV6FragHdr;
			fs = p.frag_size != 0 ? p.frag_size : ((p.mtu - pl.hdr6 - kV6FragHdr) & ~7u);
			return;
		}
	}
	head = (uint32_t)pl.ip_off + pl.hdr;
	gap = 0;
	fs = frag_fs(p, pl.hdr);
}

__device__ __forceinline__ bool is_v6_extension(uint32_t nh)
{
	return nh == 0 || nh == 43 || nh == 44 || nh == 51 || nh == 60;
}

// The plan of an IPv6 candidate: layer L of the in-bounds, selected packet at batch offset off, caplen cap. Single
// bytes are read only in [ip_off, ip_off + hdr), which the checks ahead of the walk put inside the packet. plain: every
// layer recorded ahead of it is Ethernet, VLAN or SLL (else computeCalculateFields changes more than is written here).
__device__ __forceinline__ Plan classify6(const FrIn6& p, const pcppx_layer& L, uint64_t off, uint32_t cap, bool plain)
{
	Plan pl{};
	pl.disp = PCPPX_FRAG_NOT_IP;
	if (L.hdr_len < kV6Fixed || L.hdr_len > L.data_len || (uint32_t)L.offset + L.data_len > cap)
		return pl;
	const uint32_t hdr = L.hdr_len, pay = (uint32_t)L.data_len - L.hdr_len;
	const uint8_t* ip = p.data + off + L.offset;
	uint32_t nh = ip[6], at = kV6Fixed, nh_rel = 6;
	bool fragmented = false;
#pragma unroll 1
	for (uint32_t step = 0; at < hdr; ++step)  // at most PCPPX_FRAG6_MAX_EXT + 1 trips
	{
		if (!is_v6_extension(nh) || at + 2 > hdr)
			return pl;
		if (step == PCPPX_FRAG6_MAX_EXT)
		{
			pl.disp = PCPPX_FRAG_LEFT;
			return pl;
		}
		const uint32_t len8 = ip[at + 1];
		fragmented = fragmented || nh == 44;
		nh_rel = at;
		at += nh == 44 ? 8u : nh == 51 ? (len8 + 2) * 4 : (len8 + 1) * 8;
		nh = ip[nh_rel];
	}
	if (at != hdr)
		return pl;
	pl.disp = PCPPX_FRAG_LEFT;
	if (!plain)
		return pl;
	pl.disp = PCPPX_FRAG_ALREADY;
	if (fragmented)
		return pl;
	pl.disp = PCPPX_FRAG_FITS;
	if (p.frag_size != 0 ? pay <= p.frag_size : hdr + pay <= p.mtu)
		return pl;
	pl.disp = PCPPX_FRAG_LEFT;
	if (p.frag_size == 0 && p.mtu < hdr + 2 * kV6FragHdr)
		return pl;
	pl.disp = PCPPX_FRAG_SPLIT;
	pl.ip_off = L.offset;
	pl.pay = (uint16_t)pay;
	pl.hdr6 = (uint16_t)hdr;
	pl.sum = kPlanV6 | nh_rel;
	return pl;
}

// Packet i's plan (disp kNone past the batch's end). cap: its caplen, when the descriptor is in bounds. Records that
// point outside the packet, or at no header, make it NOT_V4: nothing is read there.
__device__ __forceinline__ Plan classify(const FrIn& p, uint64_t i, uint32_t& cap)
{
	Plan pl{};
	pl.disp = kNone;
	cap = 0;
	if (i >= p.n)
		return pl;
	uint64_t off;
	pl.disp = PCPPX_FRAG_BAD_DESC;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return pl;
	pl.disp = PCPPX_FRAG_UNSELECTED;
	if (p.keep != nullptr && p.keep[i] == 0)
		return pl;
	pl.disp = PCPPX_FRAG_NOT_V4;
	const pcppx_layer* lay = p.layers + i * p.ml;
	uint32_t nl = p.n_layers[i * p.nl_stride];
	nl = nl < p.ml ? nl : p.ml;
	pcppx_layer L{};
	bool found = false;
	for (uint32_t k = 0; !found && k < nl; ++k)
	{
		L = lay[k];
		found = L.proto == kProtoIPv4;
	}
	if (!found || L.hdr_len < 20 || L.hdr_len > 60 || L.hdr_len > L.data_len || (uint32_t)L.offset + L.data_len > cap)
		return pl;
	const uint32_t hdr = L.hdr_len, pay = (uint32_t)L.data_len - L.hdr_len;
	const uint8_t* ip = p.data + off + L.offset;  // hdr >= 20 bytes of it lie inside the packet
	const uint32_t word = ((uint32_t)ip[6] << 8) | ip[7];
	pl.disp = PCPPX_FRAG_ALREADY;
	if ((word & 0x3FFFu) != 0)
		return pl;
	pl.disp = PCPPX_FRAG_FITS;
	if (p.frag_size != 0 ? pay <= p.frag_size : hdr + pay <= p.mtu)
		return pl;
	pl.disp = PCPPX_FRAG_DF;
	if (p.honor_df != 0 && (word & 0x4000u) != 0)
		return pl;
	pl.disp = PCPPX_FRAG_SPLIT;
	pl.ip_off = L.offset;
	pl.pay = (uint16_t)pay;
	pl.hdr = (uint8_t)hdr;
	// the RFC 1071 sum over the header without words 1 (total length), 3 (flags / fragment offset) and 5 (checksum):
	// every fragment adds its own; an odd last byte (no real header has one) is padded with zero
	uint32_t sum = 0;
	for (uint32_t k = 0; 2 * k < hdr; ++k)
	{
		if (k == 1 || k == 3 || k == 5)
			continue;
		sum += ((uint32_t)ip[2 * k] << 8) | (2 * k + 1 < hdr ? ip[2 * k + 1] : 0u);
	}
	pl.sum = sum;
	return pl;
}

// <true>: packet i's plan for the families asked for, from classify()'s (which knows IPv4 only; cap is its caplen).
// A packet with an IPv4 layer keeps frag's verdict, or is NOT_IP where IPv4 is not asked for; one without is taken at
// its first IPv6 layer. Kept apart from classify() so that the code of the <false> kernels stays what it was.
__device__ __forceinline__ Plan classify_families(const FrIn6& p, uint64_t i, uint32_t cap, const Plan& v4)
{
	if (v4.disp == kNone || v4.disp == PCPPX_FRAG_BAD_DESC || v4.disp == PCPPX_FRAG_UNSELECTED)
		return v4;
	Plan none{};
	none.disp = PCPPX_FRAG_NOT_IP;
	if (v4.disp != PCPPX_FRAG_NOT_V4)  // a sound IPv4 layer decided
		return (p.families & PCPPX_FRAG_FAM_V4) != 0 ? v4 : none;
	const pcppx_layer* lay = p.layers + i * p.ml;
	uint32_t nl = p.n_layers[i * p.nl_stride];
	nl = nl < p.ml ? nl : p.ml;
	pcppx_layer L6{};
	bool found6 = false, plain = true;
	for (uint32_t k = 0; k < nl; ++k)
	{
		const pcppx_layer L = lay[k];
		if (L.proto == kProtoIPv4)  // recorded, but no header inside the packet: frag's NOT_V4
			return none;
		if (!found6 && L.proto == kProtoIPv6)
		{
			L6 = L;
			found6 = true;
		}
		if (!found6)
			plain = plain && (L.proto == kProtoEth || L.proto == kProtoVlan || L.proto == kProtoSll);
	}
	return found6 ? classify6(p, L6, p.offsets[i], cap, plain) : none;
}

// the output packets and bytes of a source packet: a SPLIT packet's fragments, or the packet itself where it is copied
template <bool k6>
__device__ __forceinline__ void outputs(const FrIn& p, const Plan& pl, uint32_t cap, uint32_t& cnt, uint64_t& bytes)
{
	cnt = 0;
	bytes = 0;
	if (pl.disp == PCPPX_FRAG_SPLIT)
	{
		if constexpr (k6)
		{
			uint32_t head, gap, fs;
			split_shape<true>(p, pl, head, gap, fs);
			cnt = (pl.pay + fs - 1) / fs;  // 2..8190
			bytes = (uint64_t)cnt * (head + gap) + pl.pay;
		}
		else
		{
			const uint32_t fs = frag_fs(p, pl.hdr);
			cnt = (pl.pay + fs - 1) / fs;  // 2..8190
			bytes = (uint64_t)cnt * ((uint32_t)pl.ip_off + pl.hdr) + pl.pay;
		}
	}
	else if (pl.disp != kNone && pl.disp != PCPPX_FRAG_BAD_DESC && p.copy_rest != 0)
	{
		cnt = 1;
		bytes = cap;
	}
}

template <bool k6>
__global__ __launch_bounds__(kFrThreads) void frag_plan_kernel(In<k6> p, Plan* __restrict__ plan,
                                                               uint64_t* __restrict__ bcnt,
                                                               uint64_t* __restrict__ bbytes,
                                                               uint32_t* __restrict__ bsums)
{
	// per wave: output packets and bytes; split packets, fragments, copied, under size, bad
	__shared__ uint64_t lb[kFrWaves][2];
	__shared__ uint32_t lc[kFrWaves][kFrSums];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t c = 0, b = 0, fr = 0;
	uint32_t s[kFrSums] = { 0, 0, 0, 0, 0 };
#pragma unroll 1
	for (uint32_t u = 0; u < kFrTilesPerWave; ++u)
	{
		const uint64_t i = tile_first(kFragBlockPk, w * kFrTilesPerWave + u) + lane;
		uint32_t cap, cnt;
		uint64_t bytes;
		Plan pl = classify(p, i, cap);
		if constexpr (k6)
			pl = classify_families(p, i, cap, pl);
		if (pl.disp != kNone)
			plan[i] = pl;
		outputs<k6>(p, pl, cap, cnt, bytes);
		const bool split = pl.disp == PCPPX_FRAG_SPLIT;
		c += cnt;
		b += bytes;
		fr += split ? cnt : 0u;
		s[0] += __popcll(__ballot(split));
		s[2] += __popcll(__ballot(!split && cnt != 0));
		s[3] += __popcll(__ballot(pl.disp == PCPPX_FRAG_FITS));
		s[4] += __popcll(__ballot(pl.disp == PCPPX_FRAG_BAD_DESC));
	}
	c = wave_sum(c);
	b = wave_sum(b);
	s[1] = (uint32_t)wave_sum(fr);  // <= 1024 * 8190
	if (lane == 0)
	{
		lb[w][0] = c;
		lb[w][1] = b;
		for (uint32_t k = 0; k < kFrSums; ++k)
			lc[w][k] = s[k];
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		bcnt[blockIdx.x] = lb[0][0] + lb[1][0] + lb[2][0] + lb[3][0];
		bbytes[blockIdx.x] = lb[0][1] + lb[1][1] + lb[2][1] + lb[3][1];
		for (uint32_t k = 0; k < kFrSums; ++k)
			bsums[(uint64_t)k * gridDim.x + blockIdx.x] = lc[0][k] + lc[1][k] + lc[2][k] + lc[3][k];
	}
}

// One wave: the exclusive prefix of the g block sums (64 a step, a running carry), the totals, the verdict.
__global__ __launch_bounds__(64) void frag_base_kernel(uint32_t g, const uint64_t* __restrict__ bcnt,
                                                       const uint64_t* __restrict__ bbytes,
                                                       const uint32_t* __restrict__ bsums,
                                                       uint64_t* __restrict__ base_cnt,
                                                       uint64_t* __restrict__ base_bytes, FrOut o)
{
	const uint32_t lane = threadIdx.x;
	uint64_t run_c = 0, run_b = 0, sums[kFrSums] = { 0, 0, 0, 0, 0 };
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
		const uint64_t c = j < g ? bcnt[j] : 0ull, b = j < g ? bbytes[j] : 0ull;
#pragma unroll
		for (uint32_t k = 0; k < kFrSums; ++k)
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
	for (uint32_t k = 0; k < kFrSums; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		o.totals[PCPPX_FRAG_OUT_PACKETS] = run_c;
		o.totals[PCPPX_FRAG_OUT_BYTES] = run_b;
		o.totals[PCPPX_FRAG_SPLIT_PACKETS] = sums[0];
		o.totals[PCPPX_FRAG_FRAGMENTS] = sums[1];
		o.totals[PCPPX_FRAG_COPIED] = sums[2];
		o.totals[PCPPX_FRAG_UNDER_SIZE] = sums[3];
		o.totals[PCPPX_FRAG_BAD_DESC_N] = sums[4];
		o.totals[PCPPX_FRAG_OVERFLOW] = (run_c > o.max_packets || (o.data != nullptr && run_b > o.data_cap)) ? 1 : 0;
	}
}

// The block's source packets in LDS, for the kernels that walk its output packets: s_plan (kFragBlockPk entries; disp
// kNone past the batch's end) and the exclusive prefixes of their output packets (s_cp) and bytes (s_bp),
// kFragBlockPk + 1 entries each: the last one is the block's total. s_tc / s_tb: kFrTiles words of scratch. Ends in a
// block barrier.
template <bool k6>
__device__ __forceinline__ void block_prefix(const FrIn& p, const Plan* __restrict__ plan, Plan* s_plan, uint32_t* s_cp,
                                             uint64_t* s_bp, uint32_t* s_tc, uint64_t* s_tb)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 1
	for (uint32_t u = 0; u < kFrTilesPerWave; ++u)
	{
		const uint32_t tl = w * kFrTilesPerWave + u, slot = tl * 64 + lane;
		const uint64_t i = tile_first(kFragBlockPk, tl) + lane;
		Plan pl{};
		pl.disp = kNone;
		uint32_t cap = 0, cnt;
		uint64_t bytes;
		if (i < p.n)
		{
			pl = plan[i];
			cap = p.caplens[i];
		}
		outputs<k6>(p, pl, cap, cnt, bytes);
		s_plan[slot] = pl;
		const uint64_t ic = wave_scan_incl((uint64_t)cnt, lane), ib = wave_scan_incl(bytes, lane);
		s_cp[slot] = (uint32_t)(ic - cnt);  // a tile puts out at most 64 * 8190 packets, a block 1024 * 8190
		s_bp[slot] = ib - bytes;
		if (lane == 63)
		{
			s_tc[tl] = (uint32_t)ic;
			s_tb[tl] = ib;
		}
	}
	__syncthreads();
#pragma unroll 1
	for (uint32_t u = 0; u < kFrTilesPerWave; ++u)
	{
		const uint32_t tl = w * kFrTilesPerWave + u, slot = tl * 64 + lane;
		uint32_t bc = 0;
		uint64_t bb = 0;
		for (uint32_t x = 0; x < tl; ++x)
		{
			bc += s_tc[x];
			bb += s_tb[x];
		}
		s_cp[slot] += bc;
		s_bp[slot] += bb;
		if (slot == kFragBlockPk - 1)  // the last tile's last lane: the totals
		{
			s_cp[kFragBlockPk] = bc + s_tc[tl];
			s_bp[kFragBlockPk] = bb + s_tb[tl];
		}
	}
	__syncthreads();
}

// the source packet (0 .. kFragBlockPk - 1) of the block's output packet r: the last k with s_cp[k] <= r. r is below
// the block's total, so that packet puts out at least one; packets that put out none are passed over. Branch-free.
__device__ __forceinline__ uint32_t find_source(const uint32_t* s_cp, uint32_t r)
{
	uint32_t k = 0;
#pragma unroll
	for (uint32_t step = kFragBlockPk / 2; step != 0; step >>= 1)
		k = s_cp[k + step] <= r ? k + step : k;
	return k;
}

// ---- the tile copy of pcppx_steer.hip's copy kernel, as pcppx_defrag.hip has it: a function of 64 independent spans
// (one per lane; the chunk search and the edge copy are pcppx_move.h's) ----

// The wave's 64 spans: lane's span is len bytes from source position s0 to destination position q (positions shifted so
// that position % 16 = address % 16 from sbase / dbase); st false: no span. cp (65 entries) / dq / sa (64): the wave's
// own LDS rows. Whole destination chunks as one flattened list walked over the lanes (two aligned source granules
// funnel-shifted into one 16-B store), then every span's own head and tail bytes; spans share no chunk's bytes.
__device__ __forceinline__ void copy_spans(const uint8_t* sbase, uint8_t* dbase, uint32_t lane, bool st, uint64_t s0,
                                           uint64_t q, uint32_t len, uint64_t* cp, uint64_t* dq, uint64_t* sa)
{
	const uint64_t e = q + len;
	const uint64_t up = (q + 15) & ~15ull;
	const uint64_t he = e < up ? e : up;                   // head [q, he)
	const uint64_t dn = e & ~15ull, ts = dn > he ? dn : he;  // tail [ts, e)
	const uint64_t nfull = (st && dn > up) ? (dn - up) >> 4 : 0ull;
	const uint64_t incl = wave_scan_incl(nfull, lane);
	// the wave's own LDS rows: its LDS accesses complete in program order, so a wave-level fence (no block barrier: the
	// waves' tiles differ) orders these stores behind the previous call's loads and ahead of this call's
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	cp[lane] = incl - nfull;
	if (lane == 63)
		cp[64] = incl;
	dq[lane] = up;             // the first whole chunk
	sa[lane] = s0 + (up - q);  // and its source position
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	const uint64_t total = cp[64];
	for (uint64_t c0 = 0; c0 < total; c0 += 64 * kFrUnroll)
	{
		// kFrUnroll chunks per lane, 64 chunks apart; every chunk's two granules are loaded unconditionally (the second
		// one only when the source is not aligned like the destination), a chunk past the end loads the last one's again
		uint64_t s[kFrUnroll], cs[kFrUnroll];
		uint32_t live = 0;
#pragma unroll
		for (uint32_t x = 0; x < kFrUnroll; ++x)
		{
			const uint64_t c = c0 + 64 * x + lane;
			live |= (c < total ? 1u : 0u) << x;
			const uint64_t cc = c < total ? c : total - 1;
			const uint32_t k = find_packet(cp, cc);
			const uint64_t ahead = (cc - cp[k]) << 4;
			cs[x] = dq[k] + ahead;
			s[x] = sa[k] + ahead;
		}
		uint4 a[kFrUnroll], bb[kFrUnroll];
#pragma unroll
		for (uint32_t x = 0; x < kFrUnroll; ++x)
		{
			const uint4* gp = reinterpret_cast<const uint4*>(sbase + (s[x] & ~15ull));
			a[x] = gp[0];
			bb[x] = gp[(s[x] & 15) != 0 ? 1 : 0];
		}
#pragma unroll
		for (uint32_t x = 0; x < kFrUnroll; ++x)
			if ((live >> x) & 1)
				*reinterpret_cast<uint4*>(dbase + cs[x]) = funnel16(a[x], bb[x], (uint32_t)(s[x] & 15));
	}
	copy_edge(sbase, dbase, s0, q, st ? (uint32_t)(he - q) : 0u);
	copy_edge(sbase, dbase, s0 + (ts - q), ts, st ? (uint32_t)(e - ts) : 0u);
}

// Output packet r of the block (r below its total): its source packet k of the block, its number j among that packet's
// output packets, its byte position in the block's output, and for a fragment (fs != 0) its two spans: `head` bytes from
// the packet's start and `piece` bytes from byte src2 of the packet. A copied packet (fs == 0) is one span, its caplen.
// <true>: `gap` bytes lie between the two spans in the output (8 in an IPv6 fragment), which the patch kernel writes.
struct OutPacket
{
	uint32_t k, j, head, piece, src2, fs, gap;
	uint64_t pos;
};

template <bool k6>
__device__ __forceinline__ OutPacket out_packet(const FrIn& p, const Plan* s_plan, const uint32_t* s_cp,
                                                const uint64_t* s_bp, uint32_t r)
{
	OutPacket x{};
	x.k = find_source(s_cp, r);
	x.j = r - s_cp[x.k];
	const Plan pl = s_plan[x.k];
	x.pos = s_bp[x.k];
	if (pl.disp == PCPPX_FRAG_SPLIT)
	{
		if constexpr (k6)
			split_shape<true>(p, pl, x.head, x.gap, x.fs);
		else
		{
			x.fs = frag_fs(p, pl.hdr);
			x.head = (uint32_t)pl.ip_off + pl.hdr;
		}
		const uint32_t done = x.j * x.fs;  // < pay
		x.piece = pl.pay - done < x.fs ? pl.pay - done : x.fs;
		x.src2 = x.head + done;
		if constexpr (k6)
			x.pos += (uint64_t)x.j * (x.head + x.gap + x.fs);
		else
			x.pos += (uint64_t)x.j * (x.head + x.fs);  // the fragments before it are full
	}
	return x;
}

template <bool k6>
__global__ __launch_bounds__(kFrThreads) void frag_emit_kernel(In<k6> p, FrOut o, const Plan* __restrict__ plan,
                                                               const uint64_t* __restrict__ base_cnt,
                                                               const uint64_t* __restrict__ base_bytes)
{
	__shared__ Plan s_plan[kFragBlockPk];
	__shared__ uint32_t s_cp[kFragBlockPk + 1];
	__shared__ uint64_t s_bp[kFragBlockPk + 1];
	__shared__ uint32_t s_tc[kFrTiles];
	__shared__ uint64_t s_tb[kFrTiles];
	__shared__ uint64_t s_ccp[kFrWaves][65];  // the copy's rows
	__shared__ uint64_t s_dq[kFrWaves][64];
	__shared__ uint64_t s_sa[kFrWaves][64];
	if (o.totals[PCPPX_FRAG_OVERFLOW] != 0)  // all or nothing: the same word for every block
		return;
	block_prefix<k6>(p, plan, s_plan, s_cp, s_bp, s_tc, s_tb);
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint64_t first = tile_first(kFragBlockPk, 0);
#pragma unroll 1
	for (uint32_t u = 0; u < kFrTilesPerWave; ++u)  // the per-source columns
	{
		const uint32_t slot = (w * kFrTilesPerWave + u) * 64 + lane;
		const uint64_t i = first + slot;
		if (i >= p.n)
			continue;
		if (o.disposition != nullptr)
			o.disposition[i] = s_plan[slot].disp;
		if (o.counts != nullptr)
			o.counts[i] = (uint16_t)(s_cp[slot + 1] - s_cp[slot]);
	}
	const uint32_t total = s_cp[kFragBlockPk];
	const uint64_t rank0 = base_cnt[blockIdx.x], pos0 = base_bytes[blockIdx.x];
	const bool copy = o.data != nullptr;
	const auto [dbase, dal] = align16(o.data);  // position q (= byte position + dal) lives at dbase + q
	const auto [sbase, sal] = align16(p.data);  // the same for source positions (= batch offset + sal)
	for (uint32_t t0 = w * 64; t0 < total; t0 += kFrThreads)  // the same trips for every lane of the wave
	{
		const bool live = t0 + lane < total;
		const uint32_t r = live ? t0 + lane : total - 1;
		OutPacket x = out_packet<k6>(p, s_plan, s_cp, s_bp, r);
		const uint64_t i = first + x.k;  // < n: it puts out a packet
		const uint64_t off = p.offsets[i];
		if (x.fs == 0)
			x.head = p.caplens[i];
		const uint64_t pos = pos0 + x.pos;
		if (live)
		{
			const uint64_t rank = rank0 + r;  // < OUT_PACKETS <= max_packets
			o.offsets[rank] = pos;
			if constexpr (k6)
				o.caplens[rank] = x.head + x.gap + x.piece;
			else
				o.caplens[rank] = x.head + x.piece;
			if (o.index != nullptr)
				o.index[rank] = (uint32_t)i;
			if (o.frag_no != nullptr)
				o.frag_no[rank] = (uint16_t)x.j;
		}
		if (!copy)  // index-only (uniform over the grid)
			continue;
		copy_spans(sbase, dbase, lane, live, off + sal, pos + dal, live ? x.head : 0u, s_ccp[w], s_dq[w], s_sa[w]);
		const bool pc = live && x.piece != 0;
		if (__ballot(pc) == 0)
			continue;
		// <true>: the piece lands behind the gap; [pos + head, pos + head + gap) is in no span and so in no store here
		const uint64_t q2 = k6 ? pos + x.head + x.gap + dal : pos + x.head + dal;
		copy_spans(sbase, dbase, lane, pc, off + x.src2 + sal, q2, pc ? x.piece : 0u, s_ccp[w], s_dq[w], s_sa[w]);
	}
}

template <bool k6>
__global__ __launch_bounds__(kFrThreads) void frag_patch_kernel(In<k6> p, FrOut o, const Plan* __restrict__ plan,
                                                                const uint64_t* __restrict__ base_bytes,
                                                                const uint32_t* __restrict__ bsplit)
{
	__shared__ Plan s_plan[kFragBlockPk];
	__shared__ uint32_t s_cp[kFragBlockPk + 1];
	__shared__ uint64_t s_bp[kFragBlockPk + 1];
	__shared__ uint32_t s_tc[kFrTiles];
	__shared__ uint64_t s_tb[kFrTiles];
	if (o.totals[PCPPX_FRAG_OVERFLOW] != 0 || bsplit[blockIdx.x] == 0)  // the same for the whole block
		return;
	block_prefix<k6>(p, plan, s_plan, s_cp, s_bp, s_tc, s_tb);
	const uint32_t total = s_cp[kFragBlockPk];
	const uint64_t pos0 = base_bytes[blockIdx.x];
	for (uint32_t r = threadIdx.x; r < total; r += kFrThreads)
	{
		const OutPacket x = out_packet<k6>(p, s_plan, s_cp, s_bp, r);
		const Plan pl = s_plan[x.k];
		if (pl.disp != PCPPX_FRAG_SPLIT)
			continue;
		const uint32_t c = s_cp[x.k + 1] - s_cp[x.k];
		if constexpr (k6)
		{
			if ((pl.sum & kPlanV6) != 0)
			{
				// the fragment header (the gap, all 8 bytes), the next-header byte that now names it and the payload
				// length; the old next-header value from the source packet, the id from the caller
				const uint64_t i = tile_first(kFragBlockPk, 0) + x.k;
				const uint32_t nh_at = (uint32_t)pl.ip_off + (pl.sum & 0xFFFFu);
				const uint8_t nh_old = p.data[p.offsets[i] + nh_at];
				const uint32_t id = p.ids != nullptr ? p.ids[i] : p.id_base + (uint32_t)i;
				const uint32_t word = (x.j * x.fs) | (x.j + 1 < c ? 1u : 0u);
				const uint32_t plen = (uint32_t)pl.hdr6 - kV6Fixed + kV6FragHdr + x.piece;  // < hdr + pay <= 65535
				uint8_t* d = o.data + pos0 + x.pos;
				uint8_t* fh = d + x.head;
				fh[0] = nh_old;
				fh[1] = 0;
				fh[2] = (uint8_t)(word >> 8);
				fh[3] = (uint8_t)word;
				fh[4] = (uint8_t)(id >> 24);
				fh[5] = (uint8_t)(id >> 16);
				fh[6] = (uint8_t)(id >> 8);
				fh[7] = (uint8_t)id;
				d[nh_at] = 44;
				d[pl.ip_off + 4] = (uint8_t)(plen >> 8);
				d[pl.ip_off + 5] = (uint8_t)plen;
				// the type field ahead of every VLAN layer in front of the IPv6 header, as EthLayer's, VlanLayer's and
				// SllLayer's computeCalculateFields leave it: 0x8100, an 802.1ad tag's 0x88A8 too
				const pcppx_layer* lay = p.layers + i * p.ml;
				uint32_t nl = p.n_layers[i * p.nl_stride];
				nl = nl < p.ml ? nl : p.ml;
				for (uint32_t k = 0; k + 1 < nl && lay[k].proto != kProtoIPv6; ++k)
				{
					const pcppx_layer next = lay[k + 1];
					if (next.proto == kProtoVlan && next.offset >= 2 && next.offset <= pl.ip_off)
					{
						d[next.offset - 2] = 0x81;
						d[next.offset - 1] = 0x00;
					}
				}
				continue;
			}
		}
		const uint32_t tot_len = (uint32_t)pl.hdr + x.piece;  // <= hdr + pay <= 65535
		const uint32_t word = ((x.j * x.fs) >> 3) | (x.j + 1 < c ? 0x2000u : 0u);
		uint32_t sum = pl.sum + tot_len + word;
		while (sum >> 16)
			sum = (sum & 0xFFFFu) + (sum >> 16);
		const uint32_t ck = ~sum & 0xFFFFu;
		uint8_t* d = o.data + pos0 + x.pos + pl.ip_off;
		d[2] = (uint8_t)(tot_len >> 8);
		d[3] = (uint8_t)tot_len;
		d[6] = (uint8_t)(word >> 8);
		d[7] = (uint8_t)word;
		d[10] = (uint8_t)(ck >> 8);
		d[11] = (uint8_t)ck;
	}
}
}  // namespace

uint32_t frag_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kFragBlockPk - 1) / kFragBlockPk);
}

uint64_t frag_scratch_bytes(uint32_t n)
{
	return 52ull * frag_blocks(n) + 12ull * n;
}

int launch_frag(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* n_layers,
                uint32_t nl_stride, const pcppx_frag6_spec* spec, const pcppx_fragmented* out, void* scratch,
                hipStream_t stream)
{
	const bool k6 = (spec->families & PCPPX_FRAG_FAM_V6) != 0;
	const uint32_t g = frag_blocks(b->n);
	// bcnt, bbytes, base_cnt, base_bytes [g each, 64-bit] | five sums [g each, 32-bit] | plan[n]; 52 g + 12 n bytes
	uint64_t* bcnt = static_cast<uint64_t*>(scratch);
	uint64_t* bbytes = bcnt + g;
	uint64_t* base_cnt = bbytes + g;
	uint64_t* base_bytes = base_cnt + g;
	uint32_t* bsums = reinterpret_cast<uint32_t*>(base_bytes + g);
	Plan* plan = reinterpret_cast<Plan*>(bsums + (uint64_t)kFrSums * g);
	FrIn in{ b->data, b->offsets, b->caplens,     b->data_len, b->n,           layers,          ml,
		     n_layers, nl_stride,  spec->keep,     spec->frag_size, spec->mtu, spec->copy_rest, spec->honor_df };
	FrOut o{ out->data,    out->data_cap, out->offsets,     out->caplens,     out->index,
		     out->frag_no, out->counts,   out->disposition, out->max_packets, out->totals };
	FrIn6 in6{};
	static_cast<FrIn&>(in6) = in;
	in6.families = spec->families;
	in6.id_base = spec->id_base;
	in6.ids = spec->ids;
	const dim3 grid(g), block(kFrThreads);
	if (k6)
		hipLaunchKernelGGL(frag_plan_kernel<true>, grid, block, 0, stream, in6, plan, bcnt, bbytes, bsums);
	else
		hipLaunchKernelGGL(frag_plan_kernel<false>, grid, block, 0, stream, in, plan, bcnt, bbytes, bsums);
	hipLaunchKernelGGL(frag_base_kernel, dim3(1), dim3(64), 0, stream, g, bcnt, bbytes, bsums, base_cnt, base_bytes, o);
	if (k6)
		hipLaunchKernelGGL(frag_emit_kernel<true>, grid, block, 0, stream, in6, o, plan, base_cnt, base_bytes);
	else
		hipLaunchKernelGGL(frag_emit_kernel<false>, grid, block, 0, stream, in, o, plan, base_cnt, base_bytes);
	if (out->data != nullptr)  // bsums' first row: the blocks' split packets
	{
		if (k6)
			hipLaunchKernelGGL(frag_patch_kernel<true>, grid, block, 0, stream, in6, o, plan, base_bytes, bsums);
		else
			hipLaunchKernelGGL(frag_patch_kernel<false>, grid, block, 0, stream, in, o, plan, base_bytes, bsums);
	}
	return check_launch("frag", stream);
}
}  // namespace pcppx
