// pcppx_defrag.hip — pcppx_defrag_device / pcppx_defrag6_device: reassemble the IPv4 (and IPv6) fragment groups that are
// complete inside one batch in HBM.
//
// The contract is in include/pcppx.h (defrag, defrag6). Every kernel but the base one is a template over k6: <false> is
// pcppx_defrag_device's and pcppx_defrag6_device's with families = V4 (IPv6 fragments never enter the table), <true>
// takes the fragments of both families as candidates (a family the spec does not ask for only poisons its keys) and
// adds the IPv6 edges: the layer a candidate is, the first member's extension chain, its two pieces and its patch. Plain launches in stream order; no block waits on another, no thread
// spins: every table probe is bounded by the table's size, every list walk by PCPPX_DEFRAG_MAX_FRAGS + 1.
//   (clear)                the group table's keys, counts, list heads, maxima and in-place counts; the candidate counter
//   defrag_collect_kernel  per kDefragBlockPk-packet block: the candidates (an IPv4 fragment whose IPv4 layer is
//                          recorded). Each takes a record (one counter add per block) and joins its group: an
//                          open-addressed table keyed by ip_key (the slot is claimed by a 64-bit compare-and-swap of
//                          occupancy + key: key 0 is legal), per slot a member count, the maximum source index and a
//                          list head (atomic exchange). Which record and which slot a candidate gets depends on the
//                          order the atomics land in; nothing that is put out does: the records and lists are used as
//                          sets, the counts and maxima are sums and maxima.
//   defrag_verdict_kernel  per candidate: a walk over its group's list: the members that sort before it by
//                          (frag_offset, source index) and the sum of their len. It is in place iff that sum is its
//                          frag_offset, its len > 0 and it has F_LAST exactly when nothing sorts after it (<true>: and
//                          every member is of its family, one the spec asks for); the member nothing sorts before
//                          also checks the two size bounds (<true>, IPv6: and walks its extension chain) and notes
//                          itself and the total. A group is clean iff all of its 2..64 members are in place (a count).
//                          Quadratic in the group.
//   defrag_count_kernel    per block: output packets and bytes, reassembled / merged / left / bad packets
//   defrag_base_kernel     one wave: exclusive prefix of the block sums, the totals, the all-or-nothing verdict
//   defrag_place_kernel    exits on overflow. Per block, each wave its four 64-packet tiles: a wave scan gives the rank
//                          and 64-bit byte position of every output packet; descriptors, disposition; the copied
//                          packets' bytes (the tile copy of pcppx_steer.hip: the tile's whole destination 16-B chunks
//                          as one flattened list over the 64 lanes, then each packet's head and tail); a reassembled
//                          packet's position goes to its group's slot
//   defrag_merge_kernel    per candidate of a clean group: its piece to its place in the group's packet (the first
//                          member: its bytes up to the end of its IP payload), 64 candidates per wave, the same copy.
//                          An IPv6 group: every member's payload behind the fixed header, and in a second round of
//                          the same copy the first member's bytes up to the end of its fixed header (the extensions
//                          between the two pieces are cut)
//   defrag_patch_kernel    per clean group: total length, fragment word and header checksum of the reassembled packet
//                          (IPv6: payload length and next header), computed from the first member's source bytes (no
//                          read of what the merge kernel stored)
// All byte positions are 64-bit. Source bytes are read only through aligned 16-B granules (or single bytes) that hold
// a byte of a packet that is emitted or merged; destination bytes only inside the packet's own span.
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
constexpr uint32_t kDfThreads = 256, kDfWaves = kDfThreads / 64;
constexpr uint32_t kDfTilesPerWave = 4, kDfTiles = kDfWaves * kDfTilesPerWave;
static_assert(kDfTiles * 64 == kDefragBlockPk, "a block takes kDefragBlockPk packets");
static_assert(kDfThreads == kDefragCandPerBlock, "one thread per candidate");
static_assert(PCPPX_DEFRAG_MAX_FRAGS <= 255, "frags[] is a byte");
constexpr uint32_t kDfUnroll = 4;  // 16-B chunks a lane has in flight in the copy loop
constexpr uint32_t kProtoIPv4 = 2;  // pcpp::IPv4
constexpr uint32_t kProtoIPv6 = 3;  // pcpp::IPv6
constexpr uint32_t kV6Fixed = 40;   // sizeof(ip6_hdr)
constexpr uint32_t kDfAhead = 4;    // layer entries classify loads ahead of the chain's length
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr unsigned long long kOccupied = 1ull << 32;

enum : uint32_t
{
	kNone,    // past the batch's end
	kBad,     // descriptor out of bounds
	kPass,    // not a fragment
	kLeft,    // a fragment the device leaves to the host
	kCand,    // classify only: a candidate, its group not looked at yet
	kMerged,  // member of a clean group
	kLast     // the member whose slot holds the group's packet
};

// One candidate, 40 bytes. next: the group's list, record number + 1 (0 ends it).
struct Cand
{
	uint64_t off;  // the packet's source offset
	uint32_t idx;  // its source number
	uint32_t key;
	uint32_t next;
	uint32_t slot;
	uint16_t foff, len, ip_off, hdr;
	uint32_t flags;  // ip_status
};
static_assert(sizeof(Cand) == 40, "defrag_scratch_bytes");

struct Table
{
	uint32_t* counters;  // [0]: candidates found (may exceed room)
	unsigned long long* key64;  // per slot: 0 = free, else kOccupied | ip_key
	uint64_t* grp_pos;          // clean groups: the packet's output byte position
	uint32_t *count, *head, *maxidx, *inplace;  // members, list head (record + 1), highest source index, members in place
	uint32_t *grp_first, *grp_total;            // clean groups: the first member's record, the sum of the len
	Cand* cand;
	uint32_t room, slots, shift;  // slots = 1 << (32 - shift)
};

struct DfIn
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
	const pcppx_reasm_info* info;
	uint32_t passthrough;
	uint32_t families;  // PCPPX_DEFRAG_FAM_*: the families whose groups may be clean
};

struct DfOut
{
	uint8_t* data;  // null: index-only
	uint64_t data_cap;
	uint64_t* offsets;
	uint32_t* caplens;
	uint32_t* index;
	uint32_t* first;
	uint8_t* frags;
	uint8_t* disposition;
	uint32_t max_packets;
	uint64_t* totals;
};

// packet i: kNone / kBad / kPass / kLeft / kCand (then c holds its record but for next and slot). off / cap: its
// descriptor, when in bounds. Records that point outside the packet make it kLeft: nothing is read there.
// Dependent loads are what a fragment costs here, so they go out in two rounds: the descriptor with the status, then
// the chain's length with its first kDfAhead entries (entries past n_layers are unspecified, but inside the row) and
// the key; only a deeper IPv4 layer takes a load per entry. k6: an IPv6 fragment is a candidate by its first IPv6 layer
// (hdr: the fixed header and the extensions, at least the fragment header; len: what the records say lies behind them).
template <bool k6>
__device__ __forceinline__ uint32_t classify(const DfIn& p, uint64_t i, uint64_t& off, uint32_t& cap, Cand& c)
{
	off = 0;
	cap = 0;
	if (i >= p.n)
		return kNone;
	const uint32_t st = p.info[i].ip_status;
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return kBad;
	if ((st & 15) != PCPPX_IPR_FRAGMENT)
		return kPass;
	if (!k6 && (st & PCPPX_IPR_F_IPV6) != 0)
		return kLeft;
	const bool v6 = k6 && (st & PCPPX_IPR_F_IPV6) != 0;
	const uint32_t proto = v6 ? kProtoIPv6 : kProtoIPv4, min_hdr = v6 ? kV6Fixed + 8 : 20u;
	const pcppx_layer* lay = p.layers + i * p.ml;
	pcppx_layer ahead[kDfAhead];
#pragma unroll
	for (uint32_t k = 0; k < kDfAhead; ++k)
		ahead[k] = lay[k < p.ml ? k : 0];
	uint32_t nl = p.n_layers[i * p.nl_stride];
	const uint32_t key = p.info[i].ip_key, foff = p.info[i].frag_offset;
	nl = nl < p.ml ? nl : p.ml;
	pcppx_layer L{};
	bool found = false;
#pragma unroll
	for (uint32_t k = 0; k < kDfAhead; ++k)
		if (!found && k < nl && ahead[k].proto == proto)
		{
			L = ahead[k];
			found = true;
		}
	for (uint32_t k = kDfAhead; !found && k < nl; ++k)
	{
		L = lay[k];
		found = L.proto == proto;
	}
	if (!found || L.hdr_len < min_hdr || L.hdr_len > L.data_len || (uint32_t)L.offset + L.data_len > cap)
		return kLeft;
	c.off = off;
	c.idx = (uint32_t)i;
	c.key = key;
	c.next = 0;
	c.slot = kNoSlot;
	c.foff = (uint16_t)foff;
	c.len = (uint16_t)(L.data_len - L.hdr_len);
	c.ip_off = L.offset;
	c.hdr = L.hdr_len;
	c.flags = st;
	return kCand;
}

// key's slot: the first free one on its probe path is claimed (insert), or kNoSlot when the key is not in the table
// (lookup). At most t.slots probes.
template <bool kInsert>
__device__ __forceinline__ uint32_t slot_of(const Table& t, uint32_t key)
{
	const unsigned long long want = kOccupied | key;
	uint32_t s = (key * 0x9E3779B1u) >> t.shift;
	for (uint32_t step = 0; step < t.slots; ++step)
	{
		unsigned long long k = __hip_atomic_load(&t.key64[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (kInsert && k == 0)
		{
			k = atomicCAS(&t.key64[s], 0ull, want);
			if (k == 0)
				return s;
		}
		if (k == want)
			return s;
		if (!kInsert && k == 0)
			return kNoSlot;
		s = (s + 1) & (t.slots - 1);
	}
	return kNoSlot;
}

template <bool k6>
__global__ __launch_bounds__(kDfThreads) void defrag_collect_kernel(DfIn p, Table t)
{
	__shared__ uint32_t s_wave[kDfWaves];  // the waves' candidates
	__shared__ uint32_t s_base;            // the block's first record
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	Cand c[kDfTilesPerWave];
	uint32_t ahead[kDfTilesPerWave];  // the tile's candidates in the lanes below
	uint32_t mine = 0, tiles = 0;     // the wave's candidates so far; bit u: this lane's packet of tile u is one
#pragma unroll
	for (uint32_t u = 0; u < kDfTilesPerWave; ++u)
	{
		uint64_t off;
		uint32_t cap;
		const bool is = classify<k6>(p, tile_first(kDefragBlockPk, w * kDfTilesPerWave + u) + lane, off, cap, c[u]) == kCand;
		const uint64_t bal = __ballot(is);
		ahead[u] = mine + __popcll(bal & ((1ull << lane) - 1));
		mine += __popcll(bal);
		tiles |= (is ? 1u : 0u) << u;
	}
	if (lane == 0)
		s_wave[w] = mine;
	__syncthreads();
	// one add to the counter per block that has candidates (adds to one address take their turns: one per wave and
	// tile cost 1 ms on a 10M batch with 3% fragments). The records are a set: their order does not show.
	if (threadIdx.x == 0)
	{
		const uint32_t all = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
		s_base = all != 0 ? atomicAdd(&t.counters[0], all) : 0u;
	}
	__syncthreads();
	uint32_t base = s_base;
	for (uint32_t x = 0; x < w; ++x)
		base += s_wave[x];
#pragma unroll
	for (uint32_t u = 0; u < kDfTilesPerWave; ++u)
	{
		const uint32_t r = base + ahead[u];
		if (((tiles >> u) & 1) == 0 || r >= t.room)  // past the room: the call overflows (the base kernel sees the counter)
			continue;
		const uint32_t s = slot_of<true>(t, c[u].key);  // slots >= 2 * room: a free slot exists
		if (s != kNoSlot)
		{
			c[u].slot = s;
			atomicAdd(&t.count[s], 1u);
			atomicMax(&t.maxidx[s], c[u].idx);
			c[u].next = atomicExch(&t.head[s], r + 1);
		}
		t.cand[r] = c[u];
	}
}

// the next-header values parseExtensions (IPv6Layer.cpp:79-147) takes for an extension
__device__ __forceinline__ bool is_v6_extension(uint32_t nh)
{
	return nh == 0 || nh == 43 || nh == 44 || nh == 51 || nh == 60;
}

// parseExtensions over the extensions ip[40, hdr) of an IPv6 header at ip, hdr >= 48 bytes that all lie inside the
// packet: true iff the chain ends exactly at hdr, holds a fragment header and does not go on behind hdr (the
// reassembled packet's parse would walk on there). nh: the next-header byte of the last extension. At most
// (hdr - 40) / 8 steps (no extension is shorter than 8 bytes); only bytes of [40, hdr) are read, and byte 6.
__device__ __forceinline__ bool walk_v6_chain(const uint8_t* ip, uint32_t hdr, uint32_t& nh)
{
	nh = ip[6];
	uint32_t at = kV6Fixed;
	bool frag = false;
	for (uint32_t step = 0; step < (hdr - kV6Fixed) / 8 && at + 2 <= hdr && is_v6_extension(nh); ++step)
	{
		const uint32_t len8 = ip[at + 1];
		frag = frag || nh == 44;
		const uint32_t ext = nh == 44 ? 8u : nh == 51 ? (len8 + 2) * 4 : (len8 + 1) * 8;
		nh = ip[at];
		at += ext;
	}
	return at == hdr && frag && !is_v6_extension(nh);
}

template <bool k6>
__global__ __launch_bounds__(kDfThreads) void defrag_verdict_kernel(DfIn p, Table t)
{
	const uint32_t nc = t.counters[0];
	const uint32_t r = blockIdx.x * kDfThreads + threadIdx.x;
	if (nc > t.room || r >= nc)
		return;
	const Cand me = t.cand[r];
	const uint32_t s = me.slot;
	if (s == kNoSlot)
		return;
	const uint32_t cnt = t.count[s];
	if (cnt < 2 || cnt > PCPPX_DEFRAG_MAX_FRAGS)
		return;
	uint32_t before = 0, sum_before = 0, after = 0, total = 0, steps = 0, mixed = 0;
	uint32_t m = t.head[s];
	while (m != 0 && steps <= PCPPX_DEFRAG_MAX_FRAGS)  // at most MAX_FRAGS + 1 steps
	{
		const Cand c = t.cand[m - 1];
		total += c.len;
		if constexpr (k6)
			mixed |= (c.flags ^ me.flags) & PCPPX_IPR_F_IPV6;
		if (c.foff < me.foff || (c.foff == me.foff && c.idx < me.idx))
		{
			++before;
			sum_before += c.len;
		}
		else if (m - 1 != r)
			++after;
		m = c.next;
		++steps;
	}
	if (m != 0 || steps != cnt)  // the walk hit its bound: not clean
		return;
	bool ok = me.len > 0 && sum_before == me.foff && ((me.flags & PCPPX_IPR_F_LAST) != 0) == (after == 0);
	const bool v6 = k6 && (me.flags & PCPPX_IPR_F_IPV6) != 0;
	if constexpr (k6)  // one family, and one the spec asks for
		ok = ok && mixed == 0 && (p.families & (v6 ? PCPPX_DEFRAG_FAM_V6 : PCPPX_DEFRAG_FAM_V4)) != 0;
	if (before == 0)  // the first member: the bounds of the whole packet
	{
		ok = ok && (uint32_t)me.ip_off + me.hdr + total <= PCPPX_MAX_CAPLEN && (uint32_t)me.hdr + total <= 65535u;
		if (ok && v6)  // its extensions are what the reference will cut
		{
			uint32_t nh;
			ok = walk_v6_chain(p.data + me.off + me.ip_off, me.hdr, nh);
		}
		if (ok)
		{
			t.grp_first[s] = r;
			t.grp_total[s] = total;
		}
	}
	if (ok)
		atomicAdd(&t.inplace[s], 1u);  // a count: the order does not show
}

// packet i's part in the output: its kind (never kCand), whether it puts a packet out and of what length, and for
// kMerged / kLast its group's slot
template <bool k6>
__device__ __forceinline__ uint32_t role(const DfIn& p, const Table& t, uint64_t i, uint64_t& off, bool& emit,
                                         uint32_t& out_len, uint32_t& slot)
{
	uint32_t cap;
	Cand c;
	uint32_t kind = classify<k6>(p, i, off, cap, c);
	slot = kNoSlot;
	if (kind == kCand)
	{
		const uint32_t s = slot_of<false>(t, c.key);
		kind = kLeft;
		if (s != kNoSlot && t.inplace[s] == t.count[s])  // count >= 1; in place only with 2..64 members
		{
			kind = c.idx == t.maxidx[s] ? kLast : kMerged;
			slot = s;
		}
	}
	emit = kind == kLast || ((kind == kPass || kind == kLeft) && p.passthrough != 0);
	out_len = 0;
	if (kind == kLast)
	{
		const Cand f = t.cand[t.grp_first[slot]];
		const bool v6 = k6 && (f.flags & PCPPX_IPR_F_IPV6) != 0;  // its extensions are cut
		out_len = (uint32_t)f.ip_off + (v6 ? kV6Fixed : (uint32_t)f.hdr) + t.grp_total[slot];
	}
	else if (emit)
		out_len = cap;
	return kind;
}

template <bool k6>
__global__ __launch_bounds__(kDfThreads) void defrag_count_kernel(DfIn p, Table t, uint64_t* __restrict__ bbytes,
                                                                  uint32_t* __restrict__ bcnt,
                                                                  uint32_t* __restrict__ bsums)
{
	// per wave: output bytes; output packets, reassembled, merged, left, bad
	__shared__ uint64_t lb[kDfWaves];
	__shared__ uint32_t lc[kDfWaves][5];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const bool grouped = t.counters[0] <= t.room;  // else the groups were not formed: only the bad descriptors count
	uint64_t b = 0;
	uint32_t c[5] = { 0, 0, 0, 0, 0 };
#pragma unroll 1
	for (uint32_t u = 0; u < kDfTilesPerWave; ++u)
	{
		const uint64_t i = tile_first(kDefragBlockPk, w * kDfTilesPerWave + u) + lane;
		uint64_t off;
		uint32_t kind, out_len = 0, slot;
		bool emit = false;
		if (grouped)
			kind = role<k6>(p, t, i, off, emit, out_len, slot);
		else
		{
			uint32_t cap;
			Cand cd;
			kind = classify<k6>(p, i, off, cap, cd) == kBad ? kBad : kNone;
		}
		b += out_len;
		c[0] += __popcll(__ballot(emit));
		c[1] += __popcll(__ballot(kind == kLast));
		c[2] += __popcll(__ballot(kind == kLast || kind == kMerged));
		c[3] += __popcll(__ballot(kind == kLeft));
		c[4] += __popcll(__ballot(kind == kBad));
	}
	b = wave_sum(b);
	if (lane == 0)
	{
		lb[w] = b;
		for (uint32_t k = 0; k < 5; ++k)
			lc[w][k] = c[k];
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		bbytes[blockIdx.x] = lb[0] + lb[1] + lb[2] + lb[3];
		bcnt[blockIdx.x] = lc[0][0] + lc[1][0] + lc[2][0] + lc[3][0];
		for (uint32_t k = 1; k < 5; ++k)
			bsums[(uint64_t)(k - 1) * gridDim.x + blockIdx.x] = lc[0][k] + lc[1][k] + lc[2][k] + lc[3][k];
	}
}

// One wave: the exclusive prefix of the g block sums (64 a step, a running carry), the totals, the verdict.
__global__ __launch_bounds__(64) void defrag_base_kernel(uint32_t g, Table t, const uint64_t* __restrict__ bbytes,
                                                         const uint32_t* __restrict__ bcnt,
                                                         const uint32_t* __restrict__ bsums,
                                                         uint64_t* __restrict__ base_bytes,
                                                         uint32_t* __restrict__ base_cnt, DfOut o,
                                                         uint32_t max_fragments)
{
	const uint32_t lane = threadIdx.x;
	uint64_t run_c = 0, run_b = 0, sums[4] = { 0, 0, 0, 0 };
	for (uint32_t j0 = 0; j0 < g; j0 += 64)
	{
		const uint32_t j = j0 + lane;
		const uint64_t c = j < g ? bcnt[j] : 0u, b = j < g ? bbytes[j] : 0ull;
#pragma unroll
		for (uint32_t k = 0; k < 4; ++k)
			sums[k] += j < g ? bsums[(uint64_t)k * g + j] : 0u;
		const uint64_t ic = wave_scan_incl(c, lane), ib = wave_scan_incl(b, lane);
		if (j < g)
		{
			base_cnt[j] = (uint32_t)(run_c + ic - c);  // < the output packets <= n
			base_bytes[j] = run_b + ib - b;
		}
		run_c += __shfl(ic, 63);
		run_b += __shfl(ib, 63);
	}
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k)
		sums[k] = wave_sum(sums[k]);
	if (lane == 0)
	{
		const uint64_t nc = t.counters[0];
		o.totals[PCPPX_DEFRAG_OUT_PACKETS] = run_c;
		o.totals[PCPPX_DEFRAG_OUT_BYTES] = run_b;
		o.totals[PCPPX_DEFRAG_REASSEMBLED] = sums[0];
		o.totals[PCPPX_DEFRAG_MERGED_FRAGS] = sums[1];
		o.totals[PCPPX_DEFRAG_LEFT_FRAGS] = sums[2];
		o.totals[PCPPX_DEFRAG_CANDIDATES] = nc;
		o.totals[PCPPX_DEFRAG_BAD_DESC_N] = sums[3];
		o.totals[PCPPX_DEFRAG_OVERFLOW] =
		    (nc > max_fragments || run_c > o.max_packets || (o.data != nullptr && run_b > o.data_cap)) ? 1 : 0;
	}
}

// ---- the tile copy of pcppx_steer.hip's copy kernel, as a function of 64 independent spans (one per lane; the chunk
// search and the edge copy are pcppx_move.h's) ----

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
	for (uint64_t c0 = 0; c0 < total; c0 += 64 * kDfUnroll)
	{
		// kDfUnroll chunks per lane, 64 chunks apart; every chunk's two granules are loaded unconditionally (the second
		// one only when the source is not aligned like the destination), a chunk past the end loads the last one's again
		uint64_t s[kDfUnroll], cs[kDfUnroll];
		uint32_t live = 0;
#pragma unroll
		for (uint32_t x = 0; x < kDfUnroll; ++x)
		{
			const uint64_t c = c0 + 64 * x + lane;
			live |= (c < total ? 1u : 0u) << x;
			const uint64_t cc = c < total ? c : total - 1;
			const uint32_t k = find_packet(cp, cc);
			const uint64_t ahead = (cc - cp[k]) << 4;
			cs[x] = dq[k] + ahead;
			s[x] = sa[k] + ahead;
		}
		uint4 a[kDfUnroll], bb[kDfUnroll];
#pragma unroll
		for (uint32_t x = 0; x < kDfUnroll; ++x)
		{
			const uint4* gp = reinterpret_cast<const uint4*>(sbase + (s[x] & ~15ull));
			a[x] = gp[0];
			bb[x] = gp[(s[x] & 15) != 0 ? 1 : 0];
		}
#pragma unroll
		for (uint32_t x = 0; x < kDfUnroll; ++x)
			if ((live >> x) & 1)
				*reinterpret_cast<uint4*>(dbase + cs[x]) = funnel16(a[x], bb[x], (uint32_t)(s[x] & 15));
	}
	copy_edge(sbase, dbase, s0, q, st ? (uint32_t)(he - q) : 0u);
	copy_edge(sbase, dbase, s0 + (ts - q), ts, st ? (uint32_t)(e - ts) : 0u);
}

template <bool k6>
__global__ __launch_bounds__(kDfThreads) void defrag_place_kernel(DfIn p, Table t, DfOut o,
                                                                  const uint64_t* __restrict__ base_bytes,
                                                                  const uint32_t* __restrict__ base_cnt)
{
	__shared__ uint64_t s_cp[kDfWaves][65];
	__shared__ uint64_t s_dq[kDfWaves][64];
	__shared__ uint64_t s_sa[kDfWaves][64];
	__shared__ uint64_t s_tb[kDfTiles];  // the tiles' output bytes / packets
	__shared__ uint32_t s_tc[kDfTiles];
	// every packet's role from the first pass, for the second one (each thread reads back what it wrote: no barrier)
	__shared__ uint64_t s_off[kDfTiles][64];
	__shared__ uint32_t s_len[kDfTiles][64];
	__shared__ uint32_t s_slot[kDfTiles][64];
	__shared__ uint8_t s_kind[kDfTiles][64];  // kind | emit << 7
	if (o.totals[PCPPX_DEFRAG_OVERFLOW] != 0)  // all or nothing: the same word for every block
		return;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 1
	for (uint32_t u = 0; u < kDfTilesPerWave; ++u)
	{
		const uint32_t tl = w * kDfTilesPerWave + u;
		uint64_t off;
		uint32_t out_len, slot;
		bool emit;
		const uint32_t kind = role<k6>(p, t, tile_first(kDefragBlockPk, tl) + lane, off, emit, out_len, slot);
		s_off[tl][lane] = off;
		s_len[tl][lane] = out_len;
		s_slot[tl][lane] = slot;
		s_kind[tl][lane] = (uint8_t)(kind | (emit ? 0x80u : 0u));
		const uint64_t b = wave_sum(out_len);
		const uint32_t c = __popcll(__ballot(emit));
		if (lane == 0)
		{
			s_tb[tl] = b;
			s_tc[tl] = c;
		}
	}
	__syncthreads();
	// the wave's first tile starts behind the blocks before this one and the block's tiles before it
	uint64_t tile_pos = base_bytes[blockIdx.x], tile_rank = base_cnt[blockIdx.x];
	for (uint32_t x = 0; x < w * kDfTilesPerWave; ++x)
	{
		tile_pos += s_tb[x];
		tile_rank += s_tc[x];
	}
	const bool copy = o.data != nullptr;
	const auto [dbase, dal] = align16(o.data);  // position q (= byte position + dal) lives at dbase + q
	const auto [sbase, sal] = align16(p.data);  // the same for source positions (= batch offset + sal)
#pragma unroll 1
	for (uint32_t u = 0; u < kDfTilesPerWave; ++u)
	{
		const uint32_t tl = w * kDfTilesPerWave + u;
		const uint64_t i = tile_first(kDefragBlockPk, tl) + lane;
		const uint64_t off = s_off[tl][lane];
		const uint32_t out_len = s_len[tl][lane], slot = s_slot[tl][lane];
		const uint32_t kind = s_kind[tl][lane] & 0x7Fu;
		const bool emit = (s_kind[tl][lane] & 0x80u) != 0;
		const uint64_t bal = __ballot(emit);
		const uint32_t r = (uint32_t)tile_rank + __popcll(bal & ((1ull << lane) - 1));
		const uint64_t pos = tile_pos + wave_scan_incl(out_len, lane) - out_len;
		tile_pos += s_tb[tl];
		tile_rank += s_tc[tl];
		if (kind != kNone && o.disposition != nullptr)
			o.disposition[i] = kind == kBad      ? PCPPX_DEFRAG_BAD_DESC
			                   : kind == kPass   ? PCPPX_DEFRAG_PASS
			                   : kind == kLeft   ? PCPPX_DEFRAG_LEFT
			                   : kind == kMerged ? PCPPX_DEFRAG_MERGED
			                                     : PCPPX_DEFRAG_MERGED_LAST;
		if (emit)
		{
			o.offsets[r] = pos;
			o.caplens[r] = out_len;
			if (o.index != nullptr)
				o.index[r] = (uint32_t)i;
			if (o.first != nullptr)
				o.first[r] = kind == kLast ? t.cand[t.grp_first[slot]].idx : (uint32_t)i;
			if (o.frags != nullptr)
				o.frags[r] = kind == kLast ? (uint8_t)t.count[slot] : 0;
		}
		if (kind == kLast)
			t.grp_pos[slot] = pos;  // where the merge and patch kernels put the group's packet
		if (!copy)  // index-only (uniform over the grid)
			continue;
		const bool st = emit && kind != kLast;  // a copied packet
		if (__ballot(st) == 0)
			continue;
		copy_spans(sbase, dbase, lane, st, off + sal, pos + dal, st ? out_len : 0u, s_cp[w], s_dq[w], s_sa[w]);
	}
}

// candidate r's clean group, or kNoSlot: r past the candidates, the call overflowed, or its group stays with the host
__device__ __forceinline__ uint32_t clean_slot(const Table& t, const DfOut& o, uint32_t r, Cand& c)
{
	if (o.totals[PCPPX_DEFRAG_OVERFLOW] != 0 || r >= t.counters[0])
		return kNoSlot;
	c = t.cand[r];
	const uint32_t s = c.slot;
	return (s != kNoSlot && t.inplace[s] == t.count[s]) ? s : kNoSlot;
}

template <bool k6>
__global__ __launch_bounds__(kDfThreads) void defrag_merge_kernel(DfIn p, Table t, DfOut o)
{
	__shared__ uint64_t s_cp[kDfWaves][65];
	__shared__ uint64_t s_dq[kDfWaves][64];
	__shared__ uint64_t s_sa[kDfWaves][64];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kDfThreads + threadIdx.x;
	Cand c;
	const uint32_t s = clean_slot(t, o, r, c);
	const bool st = s != kNoSlot;
	if (__ballot(st) == 0)
		return;
	uint64_t src = 0, dst = 0, src2 = 0, dst2 = 0;
	uint32_t len = 0, len2 = 0;  // 2: the first IPv6 member's second piece
	if (st)
	{
		const uint32_t fr = t.grp_first[s];
		const Cand f = t.cand[fr];
		if (k6 && (c.flags & PCPPX_IPR_F_IPV6) != 0)  // every member's payload behind the first one's fixed header
		{
			src = c.off + c.ip_off + c.hdr;
			dst = t.grp_pos[s] + f.ip_off + kV6Fixed + c.foff;
			len = c.len;
			if (fr == r)  // and the first member's bytes up to the end of its fixed header: its extensions are cut
			{
				src2 = c.off;
				dst2 = t.grp_pos[s];
				len2 = (uint32_t)c.ip_off + kV6Fixed;
			}
		}
		else if (fr == r)  // the first member: its bytes up to the end of its IP payload (a trailer is dropped)
		{
			src = c.off;
			dst = t.grp_pos[s];
			len = (uint32_t)c.ip_off + c.hdr + c.len;
		}
		else  // in place: frag_offset + len <= total, inside the group's packet
		{
			src = c.off + c.ip_off + c.hdr;
			dst = t.grp_pos[s] + f.ip_off + f.hdr + c.foff;
			len = c.len;
		}
	}
	const auto [dbase, dal] = align16(o.data);
	const auto [sbase, sal] = align16(p.data);
	copy_spans(sbase, dbase, lane, st, src + sal, dst + dal, len, s_cp[w], s_dq[w], s_sa[w]);
	if constexpr (k6)
	{
		const bool st2 = len2 != 0;
		if (__ballot(st2) != 0)
			copy_spans(sbase, dbase, lane, st2, src2 + sal, dst2 + dal, len2, s_cp[w], s_dq[w], s_sa[w]);
	}
}

template <bool k6>
__global__ __launch_bounds__(kDfThreads) void defrag_patch_kernel(DfIn p, Table t, DfOut o)
{
	const uint32_t r = blockIdx.x * kDfThreads + threadIdx.x;
	Cand c;
	const uint32_t s = clean_slot(t, o, r, c);
	if (s == kNoSlot || t.grp_first[s] != r)
		return;
	const uint32_t tot_len = (uint32_t)c.hdr + t.grp_total[s];  // <= 65535
	const uint8_t* ip = p.data + c.off + c.ip_off;
	if (k6 && (c.flags & PCPPX_IPR_F_IPV6) != 0)
	{
		// IPReassembly.cpp:476 stores hdr + total without htobe16; the parse of :481 clamps the layer to that value read
		// as big-endian (IPv6Layer.cpp:37-39), and computeCalculateFields writes the clamped length back
		const uint32_t swapped = ((tot_len & 0xFFu) << 8) | (tot_len >> 8), total = t.grp_total[s];
		const uint32_t plen = total < swapped ? total : swapped;
		uint32_t nh;
		walk_v6_chain(ip, c.hdr, nh);  // removeAllExtensions: the last extension's next header
		uint8_t* d = o.data + t.grp_pos[s] + c.ip_off;
		d[4] = (uint8_t)(plen >> 8);
		d[5] = (uint8_t)plen;
		d[6] = (uint8_t)nh;
		return;
	}
	// the RFC 1071 sum over the header as it will stand: words 1 (total length), 3 (flags / fragment offset) and 5
	// (checksum) replaced; an odd last byte (no real header has one) is padded with zero
	uint32_t sum = tot_len;
	for (uint32_t k = 0; 2 * k < c.hdr; ++k)
	{
		if (k == 1 || k == 3 || k == 5)
			continue;
		sum += ((uint32_t)ip[2 * k] << 8) | (2 * k + 1 < c.hdr ? ip[2 * k + 1] : 0u);
	}
	while (sum >> 16)
		sum = (sum & 0xFFFFu) + (sum >> 16);
	const uint32_t ck = ~sum & 0xFFFFu;
	uint8_t* d = o.data + t.grp_pos[s] + c.ip_off;
	d[2] = (uint8_t)(tot_len >> 8);
	d[3] = (uint8_t)tot_len;
	d[6] = 0;
	d[7] = 0;
	d[10] = (uint8_t)(ck >> 8);
	d[11] = (uint8_t)ck;
}
}  // namespace

uint32_t defrag_blocks(uint32_t n)
{
	return (uint32_t)(((uint64_t)n + kDefragBlockPk - 1) / kDefragBlockPk);
}

uint32_t defrag_room(uint32_t n, uint32_t max_fragments)
{
	return (max_fragments == 0 || max_fragments > n) ? n : max_fragments;
}

uint32_t defrag_slots(uint32_t room)
{
	uint32_t c = kDefragMinSlots;
	while (c < 0x80000000u && c < 2ull * room)
		c <<= 1;
	return c;
}

uint64_t defrag_scratch_bytes(uint32_t n, uint32_t max_fragments)
{
	const uint64_t g = defrag_blocks(n), F = defrag_room(n, max_fragments), C = defrag_slots((uint32_t)F);
	return 16 + 40 * g + 40 * F + 40 * C;
}

int launch_defrag(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* n_layers,
                  uint32_t nl_stride, const pcppx_reasm_info* info, uint32_t max_fragments, uint32_t passthrough,
                  uint32_t families, const pcppx_defragged* out, void* scratch, hipStream_t stream)
{
	const uint32_t g = defrag_blocks(b->n), F = defrag_room(b->n, max_fragments), C = defrag_slots(F);
	uint32_t lg = 0;
	while ((1u << lg) < C)
		++lg;
	// counters | key64[C] | count, head, maxidx, inplace [C each] | grp_pos[C] | grp_first, grp_total [C each] | cand[F]
	// | bbytes, base_bytes [g each] | bcnt, base_cnt, four sums [g each]
	uint8_t* at = static_cast<uint8_t*>(scratch);
	Table t{};
	t.counters = reinterpret_cast<uint32_t*>(at);
	t.key64 = reinterpret_cast<unsigned long long*>(at + 16);
	t.count = reinterpret_cast<uint32_t*>(t.key64 + C);
	t.head = t.count + C;
	t.maxidx = t.head + C;
	t.inplace = t.maxidx + C;
	t.grp_pos = reinterpret_cast<uint64_t*>(t.inplace + C);
	t.grp_first = reinterpret_cast<uint32_t*>(t.grp_pos + C);
	t.grp_total = t.grp_first + C;
	t.cand = reinterpret_cast<Cand*>(t.grp_total + C);
	t.room = F;
	t.slots = C;
	t.shift = 32 - lg;
	uint64_t* bbytes = reinterpret_cast<uint64_t*>(t.cand + F);
	uint64_t* base_bytes = bbytes + g;
	uint32_t* bcnt = reinterpret_cast<uint32_t*>(base_bytes + g);
	uint32_t* base_cnt = bcnt + g;
	uint32_t* bsums = base_cnt + g;  // 4 rows of g; 16 + 40 C + 40 F + 40 g bytes in all
	// what the collect kernel adds to: the counter, the keys, and the four per-slot words behind them
	if (hipMemsetAsync(scratch, 0, 16 + 24ull * C, stream) != hipSuccess)
		return PCPPX_E_HIP;
	DfIn in{ b->data, b->offsets, b->caplens, b->data_len, b->n,        layers,
		     ml,      n_layers,   nl_stride,  info,        passthrough, families };
	DfOut o{ out->data,  out->data_cap, out->offsets,     out->caplens,     out->index,
		     out->first, out->frags,    out->disposition, out->max_packets, out->totals };
	const uint32_t gc = (F + kDefragCandPerBlock - 1) / kDefragCandPerBlock;
	const uint32_t cap = max_fragments == 0 ? b->n : max_fragments;
	// families = V4: pcppx_defrag_device's kernels; else the ones that know both families
	auto launch = [&](auto k6) {
		constexpr bool v6 = decltype(k6)::value;
		hipLaunchKernelGGL(defrag_collect_kernel<v6>, dim3(g), dim3(kDfThreads), 0, stream, in, t);
		hipLaunchKernelGGL(defrag_verdict_kernel<v6>, dim3(gc), dim3(kDfThreads), 0, stream, in, t);
		hipLaunchKernelGGL(defrag_count_kernel<v6>, dim3(g), dim3(kDfThreads), 0, stream, in, t, bbytes, bcnt, bsums);
		hipLaunchKernelGGL(defrag_base_kernel, dim3(1), dim3(64), 0, stream, g, t, bbytes, bcnt, bsums, base_bytes,
		                   base_cnt, o, cap);
		hipLaunchKernelGGL(defrag_place_kernel<v6>, dim3(g), dim3(kDfThreads), 0, stream, in, t, o, base_bytes, base_cnt);
		if (out->data != nullptr)
		{
			hipLaunchKernelGGL(defrag_merge_kernel<v6>, dim3(gc), dim3(kDfThreads), 0, stream, in, t, o);
			hipLaunchKernelGGL(defrag_patch_kernel<v6>, dim3(gc), dim3(kDfThreads), 0, stream, in, t, o);
		}
	};
	if (families == PCPPX_DEFRAG_FAM_V4)
		launch(std::false_type{});
	else
		launch(std::true_type{});
	return check_launch("defrag", stream);
}
}  // namespace pcppx
