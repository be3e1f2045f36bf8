// pcppx_tcpstream.hip — pcppx_tcpstream_device: reassemble the TCP connection sides that are clean inside one batch in HBM.
//
// The contract is in include/pcppx.h (tcpstream). Plain launches in stream order; no block waits on another, no thread
// spins: every table probe is bounded by the table's size, and nothing walks a list. Linear in the batch: a data
// member's place in its stream is rel itself, so nothing is sorted; the tiling is verified through a table of segment
// starts.
//   (clear)                  the tables' keys, sums, counts and flags to 0; the minima to all ones
//   tcps_collect_kernel      per kTcpsBlockPk-packet block: every packet's kind (one word per packet); a candidate takes
//                            a record (one counter add per block) and joins its connection: an open-addressed table
//                            keyed by hash5 (a slot is claimed by a 64-bit compare-and-swap of occupancy + key: key 0
//                            is legal), per slot the minimum of (source index, record): side 0's first member
//   tcps_second_kernel       per candidate: one that differs from side 0 in (family, address, port) offers itself as
//                            side 1's first member (a minimum)
//   tcps_join_kernel         per candidate: its side (0, 1 or neither) and rel from the side's first member; per side the
//                            sum of len, the data members, their highest index (added once per wave and side), the
//                            lowest FIN / RST index, the flags seen; per connection the lowest RST index; a data
//                            member's (side, rel) goes into the segment table (open-addressed, claimed by
//                            compare-and-swap; meeting its own key: a duplicate)
//   tcps_chain_kernel        per data member: its end (side, rel + len) is looked up: found, the successor's index must
//                            be higher or the side is out of order; not found, it must be the side's sum. With a
//                            member at rel 0, no duplicate and every rel and the sum below 2^31 that is an exact tiling
//                            (the chain from 0 through the found ends stops at the sum and already adds up to it)
//   tcps_verdict_kernel      per side (its first member's thread): conditions 1-6
//   tcps_count_kernel        per block: streams and bytes (at the clean sides' first members), STREAM / LEFT / HOST / BAD
//   tcps_base_kernel         one wave: exclusive prefix of the block sums, the totals, the all-or-nothing verdict
//   tcps_place_kernel        exits on overflow. A wave scan per 64-packet tile gives every stream's record number and
//                            64-bit position, kept in its side's slot; disposition; the columns of the packets of no stream
//   tcps_emit_kernel         exits on overflow. Per candidate of a clean side: seg_stream / seg_pos; the first member
//                            writes the stream's record; the payload to pos + rel, 64 spans per wave (the copy of
//                            pcppx_defrag.hip's merge kernel over pcppx_move.h's pieces)
// Which record and which slot a candidate gets depends on the order the atomics land in; nothing that is put out does:
// records and slots are used as sets, everything else is a sum, a minimum or a maximum. All byte positions are 64-bit.
// Source bytes are read only as single header bytes of an in-bounds candidate or through aligned 16-B granules that
// hold a byte of an emitted payload; destination bytes only inside the payload's own span.
#include <hip/hip_runtime.h>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_move.h"

namespace pcppx
{
namespace
{
using namespace move;
constexpr uint32_t kTsThreads = 256, kTsWaves = kTsThreads / 64;
constexpr uint32_t kTsTilesPerWave = 4, kTsTiles = kTsWaves * kTsTilesPerWave;
static_assert(kTsTiles * 64 == kTcpsBlockPk, "a block takes kTcpsBlockPk packets");
static_assert(kTsThreads == kTcpsCandPerBlock, "one thread per candidate");
constexpr uint32_t kTsUnroll = 4;  // 16-B chunks a lane has in flight in the copy loop
constexpr uint32_t kProtoIPv4 = 2, kProtoIPv6 = 3, kProtoTcp = 4;  // pcpp::IPv4, IPv6, TCP
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kKindBase = 0xFFFFFFF0u;  // the per-packet word: a record number below it, else kKindBase + kind
constexpr unsigned long long kOccupied = 1ull << 32;
constexpr uint8_t kNoSide = 0xFF;

enum : uint32_t
{
	kNone,    // past the batch's end
	kBad,     // descriptor out of bounds
	kNotTcp,  // status other than DATA / HOST
	kHost,    // status HOST
	kLeft,    // a DATA packet the device leaves to the host
	kCand,    // classify only: a candidate
	kStream,  // data member of a clean side
	kControl  // zero-length member of a clean side
};

// a side's flags word: PCPPX_TCPS_F_* and
constexpr uint32_t kSideBad = 0x10;   // conditions 1 / 2 failed
constexpr uint32_t kSideZero = 0x20;  // a data member at rel 0

// One candidate, 64 bytes.
struct Cand
{
	uint64_t off;  // the packet's source offset
	uint32_t idx;  // its source number
	uint32_t key;  // hash5
	uint32_t slot;
	uint32_t seq;
	uint32_t len;  // info.tcp_payload
	uint32_t pay;  // the payload's offset in the packet
	uint32_t rel;
	uint16_t port;  // raw bytes
	uint8_t st;     // tcp_status
	uint8_t fam;    // 4 / 6
	uint8_t side;   // 0 / 1 / kNoSide
	uint8_t pad[3];
	uint32_t addr[4];
	uint32_t pad2;
};
static_assert(sizeof(Cand) == 64, "tcpstream_scratch_bytes");

struct Table
{
	uint32_t* counters;  // [0]: candidates found (may exceed room)
	unsigned long long* key64;   // per connection slot: 0 = free, else kOccupied | hash5
	unsigned long long* segkey;  // per segment slot: 0 = free, else ((side slot << 32) | rel) + 1
	unsigned long long* sum_len;    // per side (2 * slot + side): the sum of len
	unsigned long long* min_first;  // per side: min of (source index << 32 | record) over the members that open it
	uint64_t* pos;                  // clean sides: the stream's byte position
	uint32_t *n_data, *max_data, *flags, *clean;  // per side: data members, their highest index, flags seen, verdict
	uint32_t *min_fin, *rank;                     // per side: lowest FIN / RST index; clean sides: the record number
	uint32_t* min_rst;                            // per connection: lowest RST index
	uint32_t* segidx;                             // per segment slot: the member's source index
	uint32_t* rec_of;                             // per packet
	Cand* cand;
	uint32_t room, slots, shift;  // slots = 1 << (32 - shift)
};

struct TsIn
{
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	uint64_t data_len;
	uint32_t n;
	const pcppx_layer* layers;
	uint32_t ml;
	const uint8_t* rec0;  // packet 0's summary or brief
	uint32_t rec_stride;
	const pcppx_reasm_info* info;
	uint32_t base_clear;
};

struct TsOut
{
	uint8_t* data;  // null: index-only
	uint64_t data_cap;
	pcppx_tcpstream_rec* streams;
	uint8_t* disposition;
	uint32_t* seg_stream;
	uint32_t* seg_pos;
	uint32_t max_streams;
	uint64_t* totals;
};

// packet i: kNone / kBad / kNotTcp / kHost / kLeft / kCand (then c holds its record but for slot, rel and side).
// Records that point outside the packet make it kLeft: nothing is read there.
__device__ __forceinline__ uint32_t classify(const TsIn& p, uint64_t i, Cand& c)
{
	if (i >= p.n)
		return kNone;
	uint64_t off;
	uint32_t cap;
	const pcppx_reasm_info inf = p.info[i];
	if (out_of_bounds(p.offsets, p.caplens, p.data_len, 0, i, off, cap))
		return kBad;
	if ((inf.tcp_status & 15) == PCPPX_TCPR_HOST)
		return kHost;
	if ((inf.tcp_status & 15) != PCPPX_TCPR_DATA)
		return kNotTcp;
	const uint8_t* rec = p.rec0 + i * p.rec_stride;
	const uint32_t key = *reinterpret_cast<const uint32_t*>(rec);
	uint32_t nl = rec[14];
	const uint32_t l4 = rec[15];
	nl = nl < p.ml ? nl : p.ml;
	if (l4 >= nl)
		return kLeft;
	const pcppx_layer* lay = p.layers + i * p.ml;
	const pcppx_layer T = lay[l4];
	if (T.proto != kProtoTcp || (uint32_t)T.offset + 20 > cap ||
	    (uint64_t)T.offset + T.hdr_len + inf.tcp_payload > cap)
		return kLeft;
	uint32_t fam = 0, ip_off = 0;
	for (uint32_t k = 0; k < nl && fam == 0; ++k)
	{
		const pcppx_layer L = lay[k];
		if (L.proto == kProtoIPv4 || L.proto == kProtoIPv6)
		{
			fam = L.proto == kProtoIPv4 ? 4 : 6;
			ip_off = L.offset;
		}
	}
	if (fam == 0 || ip_off + (fam == 4 ? 16u : 24u) > cap)
		return kLeft;
	const uint8_t* pk = p.data + off;
	const uint8_t* t = pk + T.offset;
	const uint8_t* a = pk + ip_off + (fam == 4 ? 12 : 8);
	c.off = off;
	c.idx = (uint32_t)i;
	c.key = key;
	c.slot = kNoSlot;
	c.seq = ((uint32_t)t[4] << 24) | ((uint32_t)t[5] << 16) | ((uint32_t)t[6] << 8) | t[7];
	c.len = inf.tcp_payload;
	c.pay = (uint32_t)T.offset + T.hdr_len;
	c.rel = 0;
	c.port = (uint16_t)(t[0] | (t[1] << 8));
	c.st = inf.tcp_status;
	c.fam = (uint8_t)fam;
	c.side = kNoSide;
	c.pad[0] = c.pad[1] = c.pad[2] = 0;
	c.pad2 = 0;
	const uint32_t words = fam == 4 ? 1 : 4;
#pragma unroll
	for (uint32_t k = 0; k < 4; ++k)
		c.addr[k] = k < words ? (uint32_t)a[4 * k] | ((uint32_t)a[4 * k + 1] << 8) | ((uint32_t)a[4 * k + 2] << 16) |
		                            ((uint32_t)a[4 * k + 3] << 24)
		                      : 0u;
	return kCand;
}

__device__ __forceinline__ bool same_source(const Cand& x, const Cand& y)
{
	return x.fam == y.fam && x.port == y.port && x.addr[0] == y.addr[0] && x.addr[1] == y.addr[1] &&
	       x.addr[2] == y.addr[2] && x.addr[3] == y.addr[3];
}

// want's slot in an open-addressed table of 64-bit words (0 = free): the first free one on its probe path is claimed
// (insert; fresh tells whether this call claimed it), or kNoSlot when want is not in the table (lookup). At most
// t.slots probes.
template <bool kInsert>
__device__ __forceinline__ uint32_t slot_of(const Table& t, unsigned long long* keys, unsigned long long want,
                                            uint32_t hash, bool& fresh)
{
	fresh = false;
	uint32_t s = (hash * 0x9E3779B1u) >> t.shift;
	for (uint32_t step = 0; step < t.slots; ++step)
	{
		unsigned long long k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (kInsert && k == 0)
		{
			k = atomicCAS(&keys[s], 0ull, want);
			if (k == 0)
			{
				fresh = true;
				return s;
			}
		}
		if (k == want)
			return s;
		if (!kInsert && k == 0)
			return kNoSlot;
		s = (s + 1) & (t.slots - 1);
	}
	return kNoSlot;
}

// a minimum over many offers to one word: the atomic is issued only when the word read is still above the offer (the
// word only falls, so an offer at or above what was read changes nothing). A connection's candidates come roughly in
// index order, so all but its first few skip the atomic: an elephant's members would otherwise take their turns at
// one address.
__device__ __forceinline__ void offer_min(unsigned long long* w, unsigned long long v)
{
	if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v)
		atomicMin(w, v);
}
__device__ __forceinline__ void offer_min(uint32_t* w, uint32_t v)
{
	if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > v)
		atomicMin(w, v);
}

// the segment table's word for a data member of side sid at rel (< 2^31), and where its probe path starts
__device__ __forceinline__ unsigned long long seg_word(uint32_t sid, uint32_t rel)
{
	return (((unsigned long long)sid << 32) | rel) + 1;
}
__device__ __forceinline__ uint32_t seg_hash(uint32_t sid, uint32_t rel)
{
	return sid * 0x85EBCA6Bu + rel;
}

__global__ __launch_bounds__(kTsThreads) void tcps_collect_kernel(TsIn p, Table t)
{
	__shared__ uint32_t s_wave[kTsWaves];  // the waves' candidates
	__shared__ uint32_t s_base;            // the block's first record
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t kind[kTsTilesPerWave], ahead[kTsTilesPerWave];  // ahead: the wave's candidates before this lane's
	uint32_t mine = 0;
#pragma unroll 1
	for (uint32_t u = 0; u < kTsTilesPerWave; ++u)
	{
		Cand c;
		kind[u] = classify(p, tile_first(kTcpsBlockPk, w * kTsTilesPerWave + u) + lane, c);
		const uint64_t bal = __ballot(kind[u] == kCand);
		ahead[u] = mine + __popcll(bal & ((1ull << lane) - 1));
		mine += __popcll(bal);
	}
	if (lane == 0)
		s_wave[w] = mine;
	__syncthreads();
	// one add to the counter per block that has candidates; the records are a set: their order does not show
	if (threadIdx.x == 0)
	{
		const uint32_t all = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
		s_base = all != 0 ? atomicAdd(&t.counters[0], all) : 0u;
	}
	__syncthreads();
	uint32_t base = s_base;
	for (uint32_t x = 0; x < w; ++x)
		base += s_wave[x];
#pragma unroll 1
	for (uint32_t u = 0; u < kTsTilesPerWave; ++u)
	{
		const uint64_t i = tile_first(kTcpsBlockPk, w * kTsTilesPerWave + u) + lane;
		if (kind[u] == kNone)
			continue;
		const uint32_t r = base + ahead[u];
		if (kind[u] != kCand || r >= t.room)  // past the room: the call overflows (the base kernel sees the counter)
		{
			t.rec_of[i] = kKindBase + (kind[u] == kCand ? (uint32_t)kLeft : kind[u]);
			continue;
		}
		Cand c;
		classify(p, i, c);  // again, rather than four records held in registers over the barrier
		bool fresh;
		const uint32_t s = slot_of<true>(t, t.key64, kOccupied | c.key, c.key, fresh);  // slots >= 2 * room
		if (s != kNoSlot)
		{
			c.slot = s;
			offer_min(&t.min_first[2ull * s], ((unsigned long long)c.idx << 32) | r);
		}
		t.cand[r] = c;
		t.rec_of[i] = r;
	}
}

// candidate r, when the connections were formed and it has one; nc: the candidates
__device__ __forceinline__ bool load_cand(const Table& t, uint32_t r, Cand& c)
{
	const uint32_t nc = t.counters[0];
	if (nc > t.room || r >= nc)
		return false;
	c = t.cand[r];
	return c.slot != kNoSlot;
}

__global__ __launch_bounds__(kTsThreads) void tcps_second_kernel(Table t)
{
	const uint32_t r = blockIdx.x * kTsThreads + threadIdx.x;
	Cand c;
	if (!load_cand(t, r, c))
		return;
	const Cand c0 = t.cand[(uint32_t)t.min_first[2ull * c.slot]];
	if (!same_source(c, c0))
		offer_min(&t.min_first[2ull * c.slot + 1], ((unsigned long long)c.idx << 32) | r);
}

__global__ __launch_bounds__(kTsThreads) void tcps_join_kernel(Table t)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t r = blockIdx.x * kTsThreads + threadIdx.x;
	Cand c{};
	bool joined = load_cand(t, r, c);  // no lane leaves before the wave's sums below
	uint32_t side = 0, sid = 0, rel = 0;
	if (joined)
	{
		Cand f = t.cand[(uint32_t)t.min_first[2ull * c.slot]];
		if (!same_source(c, f))
		{
			// it differs from side 0, so side 1 has a first member (this one offered itself)
			f = t.cand[(uint32_t)t.min_first[2ull * c.slot + 1]];
			side = 1;
			joined = same_source(c, f);  // else a third source: LEFT (its record keeps kNoSide)
		}
		sid = 2 * c.slot + side;
		rel = c.seq - (f.seq + ((f.st & PCPPX_TCPR_F_SYN) ? 1u : 0u));
	}
	const bool data = joined && c.len > 0;
	if (joined)
	{
		uint32_t fl = ((c.st & PCPPX_TCPR_F_SYN) ? PCPPX_TCPS_F_SYN : 0u) |
		              ((c.st & PCPPX_TCPR_F_FIN) ? PCPPX_TCPS_F_FIN : 0u) | ((c.st & PCPPX_TCPR_F_RST) ? PCPPX_TCPS_F_RST : 0u);
		if (c.st & (PCPPX_TCPR_F_FIN | PCPPX_TCPR_F_RST))
			offer_min(&t.min_fin[sid], c.idx);
		if (c.st & PCPPX_TCPR_F_RST)
			offer_min(&t.min_rst[c.slot], c.idx);
		if (data)
		{
			if (c.st & PCPPX_TCPR_F_SYN)
				fl |= kSideBad;
			if (rel >= 0x80000000u)
				fl |= kSideBad;
			else
			{
				if (rel == 0)
					fl |= kSideZero;
				bool fresh;
				const uint32_t g = slot_of<true>(t, t.segkey, seg_word(sid, rel), seg_hash(sid, rel), fresh);
				if (g == kNoSlot || !fresh)  // a duplicate start (or no slot: never with slots >= 2 * room)
					fl |= kSideBad;
				else
					t.segidx[g] = c.idx;
			}
		}
		if (fl != 0)
			atomicOr(&t.flags[sid], fl);
		t.cand[r].rel = rel;
		t.cand[r].side = (uint8_t)side;
	}
	// the side's sum of len, data members and their highest index: the wave's lanes of one side add once (side by side,
	// at most 64 rounds), since the members of an elephant side would otherwise take their turns at one address
	uint64_t rest = __ballot(data);
	while (rest != 0)
	{
		const uint32_t leader = (uint32_t)__ffsll((unsigned long long)rest) - 1;
		const uint32_t lsid = __shfl(sid, leader);
		const bool in = data && sid == lsid;
		const uint64_t mask = __ballot(in);
		rest &= ~mask;
		uint64_t sum = c.len;
		uint32_t last = c.idx;
		if (mask != (1ull << leader))  // more than the leader: the side's lanes summed
		{
			sum = wave_sum(in ? (uint64_t)c.len : 0ull);
			last = in ? c.idx : 0u;
			for (int o = 32; o > 0; o >>= 1)
			{
				const uint32_t other = __shfl_xor(last, o);
				last = other > last ? other : last;
			}
		}
		if (lane == leader)
		{
			atomicAdd(&t.sum_len[lsid], (unsigned long long)sum);
			atomicAdd(&t.n_data[lsid], (uint32_t)__popcll(mask));
			atomicMax(&t.max_data[lsid], last);
		}
	}
}

__global__ __launch_bounds__(kTsThreads) void tcps_chain_kernel(Table t)
{
	const uint32_t r = blockIdx.x * kTsThreads + threadIdx.x;
	Cand c;
	if (!load_cand(t, r, c) || c.side == kNoSide || c.len == 0 || c.rel >= 0x80000000u)
		return;
	const uint32_t sid = 2 * c.slot + c.side;
	const uint64_t end = (uint64_t)c.rel + c.len;
	uint32_t fl = 0;
	if (end >= 0x80000000ull)  // the total is at least end
		fl = kSideBad;
	else
	{
		bool fresh;
		const uint32_t g = slot_of<false>(t, t.segkey, seg_word(sid, (uint32_t)end), seg_hash(sid, (uint32_t)end), fresh);
		if (g != kNoSlot)
			fl = t.segidx[g] < c.idx ? (uint32_t)PCPPX_TCPS_F_OOO : 0u;
		else if (end != t.sum_len[sid])
			fl = kSideBad;
	}
	if (fl != 0)
		atomicOr(&t.flags[sid], fl);
}

__global__ __launch_bounds__(kTsThreads) void tcps_verdict_kernel(Table t, uint32_t base_clear)
{
	const uint32_t r = blockIdx.x * kTsThreads + threadIdx.x;
	Cand c;
	if (!load_cand(t, r, c) || c.side == kNoSide)
		return;
	const uint32_t sid = 2 * c.slot + c.side, oid = sid ^ 1;
	if ((uint32_t)t.min_first[sid] != r)  // the side's first member judges it
		return;
	const uint32_t fl = t.flags[sid], nd = t.n_data[sid], last = t.max_data[sid];
	bool ok = nd > 0 && (fl & kSideBad) == 0 && (fl & kSideZero) != 0 && t.sum_len[sid] < 0x80000000ull;
	ok = ok && t.min_fin[sid] >= last;
	const unsigned long long of = t.min_first[oid];
	uint32_t other_data = 0, other_last = 0;
	if (of != ~0ull)
	{
		other_data = t.n_data[oid];
		other_last = other_data > 0 ? t.max_data[oid] : 0u;
		if (other_data > 0 && t.cand[(uint32_t)of].len > 0)
			--other_data;  // the other side's own first member never triggers the flush
	}
	ok = ok && t.min_rst[c.slot] >= (last > other_last ? last : other_last);
	ok = ok && (base_clear == 0 || (fl & PCPPX_TCPS_F_OOO) == 0 || other_data == 0);
	t.clean[sid] = ok ? 1u : 0u;
}

// packet i's part in the output: its kind (never kCand); for a member of a clean side, sid and its record; first: it
// is the side's first member, whose slot in the scan carries the stream
__device__ __forceinline__ uint32_t role(const Table& t, uint32_t n, uint64_t i, uint32_t& sid, uint32_t& rel, bool& first)
{
	first = false;
	sid = 0;
	rel = 0;
	if (i >= n)
		return kNone;
	const uint32_t r = t.rec_of[i];
	if (r >= kKindBase)
		return r - kKindBase;
	const Cand c = t.cand[r];
	if (c.slot == kNoSlot || c.side == kNoSide)
		return kLeft;
	sid = 2 * c.slot + c.side;
	if (t.clean[sid] == 0)
		return kLeft;
	rel = c.rel;
	first = (uint32_t)t.min_first[sid] == r;
	return c.len > 0 ? kStream : kControl;
}

__global__ __launch_bounds__(kTsThreads) void tcps_count_kernel(uint32_t n, Table t, uint64_t* __restrict__ bbytes,
                                                                uint32_t* __restrict__ bcnt,
                                                                uint32_t* __restrict__ bsums)
{
	// per wave: stream bytes; streams, STREAM, LEFT, HOST, BAD packets
	__shared__ uint64_t lb[kTsWaves];
	__shared__ uint32_t lc[kTsWaves][5];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const bool grouped = t.counters[0] <= t.room;  // else no connection was formed: only HOST and BAD count
	uint64_t b = 0;
	uint32_t c[5] = { 0, 0, 0, 0, 0 };
#pragma unroll 1
	for (uint32_t u = 0; u < kTsTilesPerWave; ++u)
	{
		const uint64_t i = tile_first(kTcpsBlockPk, w * kTsTilesPerWave + u) + lane;
		uint32_t kind, sid, rel;
		bool first = false;
		if (grouped)
			kind = role(t, n, i, sid, rel, first);
		else
		{
			const uint32_t r = i < n ? t.rec_of[i] : kKindBase + kNone;
			kind = r == kKindBase + kBad ? kBad : r == kKindBase + kHost ? kHost : kNone;
		}
		b += first ? t.sum_len[sid] : 0ull;
		c[0] += __popcll(__ballot(first));
		c[1] += __popcll(__ballot(kind == kStream));
		c[2] += __popcll(__ballot(kind == kLeft));
		c[3] += __popcll(__ballot(kind == kHost));
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
__global__ __launch_bounds__(64) void tcps_base_kernel(uint32_t g, Table t, const uint64_t* __restrict__ bbytes,
                                                       const uint32_t* __restrict__ bcnt,
                                                       const uint32_t* __restrict__ bsums,
                                                       uint64_t* __restrict__ base_bytes,
                                                       uint32_t* __restrict__ base_cnt, TsOut o, uint32_t max_segments)
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
			base_cnt[j] = (uint32_t)(run_c + ic - c);  // < the streams <= n
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
		o.totals[PCPPX_TCPS_STREAMS] = run_c;
		o.totals[PCPPX_TCPS_BYTES] = run_b;
		o.totals[PCPPX_TCPS_SEGMENTS] = sums[0];
		o.totals[PCPPX_TCPS_LEFT_N] = sums[1];
		o.totals[PCPPX_TCPS_CANDIDATES] = nc;
		o.totals[PCPPX_TCPS_HOST_N] = sums[2];
		o.totals[PCPPX_TCPS_BAD_DESC_N] = sums[3];
		o.totals[PCPPX_TCPS_OVERFLOW] =
		    (nc > max_segments || run_c > o.max_streams || (o.data != nullptr && run_b > o.data_cap)) ? 1 : 0;
	}
}

__global__ __launch_bounds__(kTsThreads) void tcps_place_kernel(uint32_t n, Table t, TsOut o,
                                                                const uint64_t* __restrict__ base_bytes,
                                                                const uint32_t* __restrict__ base_cnt)
{
	__shared__ uint64_t s_tb[kTsTiles];  // the tiles' stream bytes / streams
	__shared__ uint32_t s_tc[kTsTiles];
	if (o.totals[PCPPX_TCPS_OVERFLOW] != 0)  // all or nothing: the same word for every block
		return;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t kind[kTsTilesPerWave], sid[kTsTilesPerWave];
	uint64_t bytes[kTsTilesPerWave];
	uint32_t firsts = 0;  // bit u: this lane's packet of tile u carries a stream
#pragma unroll
	for (uint32_t u = 0; u < kTsTilesPerWave; ++u)
	{
		const uint32_t tl = w * kTsTilesPerWave + u;
		uint32_t rel;
		bool first;
		kind[u] = role(t, n, tile_first(kTcpsBlockPk, tl) + lane, sid[u], rel, first);
		bytes[u] = first ? t.sum_len[sid[u]] : 0ull;
		firsts |= (first ? 1u : 0u) << u;
		const uint64_t b = wave_sum(bytes[u]);
		const uint32_t c = __popcll(__ballot(first));
		if (lane == 0)
		{
			s_tb[tl] = b;
			s_tc[tl] = c;
		}
	}
	__syncthreads();
	// the wave's first tile starts behind the blocks before this one and the block's tiles before it
	uint64_t tile_pos = base_bytes[blockIdx.x], tile_rank = base_cnt[blockIdx.x];
	for (uint32_t x = 0; x < w * kTsTilesPerWave; ++x)
	{
		tile_pos += s_tb[x];
		tile_rank += s_tc[x];
	}
#pragma unroll
	for (uint32_t u = 0; u < kTsTilesPerWave; ++u)
	{
		const uint32_t tl = w * kTsTilesPerWave + u;
		const uint64_t i = tile_first(kTcpsBlockPk, tl) + lane;
		const bool first = ((firsts >> u) & 1) != 0;
		const uint64_t bal = __ballot(first);
		const uint32_t rk = (uint32_t)tile_rank + __popcll(bal & ((1ull << lane) - 1));
		const uint64_t pos = tile_pos + wave_scan_incl(bytes[u], lane) - bytes[u];
		tile_pos += s_tb[tl];
		tile_rank += s_tc[tl];
		if (first)  // where the emit kernel puts the side's stream and record
		{
			t.rank[sid[u]] = rk;
			t.pos[sid[u]] = pos;
		}
		if (kind[u] == kNone)
			continue;
		if (o.disposition != nullptr)
			o.disposition[i] = kind[u] == kBad       ? PCPPX_TCPS_BAD_DESC
			                   : kind[u] == kNotTcp  ? PCPPX_TCPS_NOT_TCP
			                   : kind[u] == kHost    ? PCPPX_TCPS_HOST
			                   : kind[u] == kLeft    ? PCPPX_TCPS_LEFT
			                   : kind[u] == kStream  ? PCPPX_TCPS_STREAM
			                                         : PCPPX_TCPS_CONTROL;
		if (kind[u] != kStream && kind[u] != kControl)  // the members' entries are the emit kernel's
		{
			if (o.seg_stream != nullptr)
				o.seg_stream[i] = PCPPX_TCPS_NONE;
			if (o.seg_pos != nullptr)
				o.seg_pos[i] = 0;
		}
	}
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
	// waves' spans differ) orders these stores ahead of this call's loads
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
	for (uint64_t c0 = 0; c0 < total; c0 += 64 * kTsUnroll)
	{
		// kTsUnroll chunks per lane, 64 chunks apart; every chunk's two granules are loaded unconditionally (the second
		// one only when the source is not aligned like the destination), a chunk past the end loads the last one's again
		uint64_t s[kTsUnroll], cs[kTsUnroll];
		uint32_t live = 0;
#pragma unroll
		for (uint32_t x = 0; x < kTsUnroll; ++x)
		{
			const uint64_t c = c0 + 64 * x + lane;
			live |= (c < total ? 1u : 0u) << x;
			const uint64_t cc = c < total ? c : total - 1;
			const uint32_t k = find_packet(cp, cc);
			const uint64_t ahead = (cc - cp[k]) << 4;
			cs[x] = dq[k] + ahead;
			s[x] = sa[k] + ahead;
		}
		uint4 a[kTsUnroll], bb[kTsUnroll];
#pragma unroll
		for (uint32_t x = 0; x < kTsUnroll; ++x)
		{
			const uint4* gp = reinterpret_cast<const uint4*>(sbase + (s[x] & ~15ull));
			a[x] = gp[0];
			bb[x] = gp[(s[x] & 15) != 0 ? 1 : 0];
		}
#pragma unroll
		for (uint32_t x = 0; x < kTsUnroll; ++x)
			if ((live >> x) & 1)
				*reinterpret_cast<uint4*>(dbase + cs[x]) = funnel16(a[x], bb[x], (uint32_t)(s[x] & 15));
	}
	copy_edge(sbase, dbase, s0, q, st ? (uint32_t)(he - q) : 0u);
	copy_edge(sbase, dbase, s0 + (ts - q), ts, st ? (uint32_t)(e - ts) : 0u);
}

__global__ __launch_bounds__(kTsThreads) void tcps_emit_kernel(const uint8_t* src, Table t, TsOut o)
{
	__shared__ uint64_t s_cp[kTsWaves][65];
	__shared__ uint64_t s_dq[kTsWaves][64];
	__shared__ uint64_t s_sa[kTsWaves][64];
	if (o.totals[PCPPX_TCPS_OVERFLOW] != 0)
		return;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kTsThreads + threadIdx.x;
	Cand c;
	bool member = load_cand(t, r, c) && c.side != kNoSide;
	uint32_t sid = 0;
	if (member)
	{
		sid = 2 * c.slot + c.side;
		member = t.clean[sid] != 0;
	}
	uint64_t pos = 0;
	if (member)
	{
		const uint32_t rk = t.rank[sid];
		pos = t.pos[sid];
		if (o.seg_stream != nullptr)
			o.seg_stream[c.idx] = rk;
		if (o.seg_pos != nullptr)
			o.seg_pos[c.idx] = c.rel;
		if ((uint32_t)t.min_first[sid] == r)
		{
			pcppx_tcpstream_rec rec{};
			rec.pos = pos;
			rec.bytes = (uint32_t)t.sum_len[sid];
			rec.flow_key = c.key;
			rec.first = c.idx;
			rec.segments = t.n_data[sid];
			rec.peer = t.clean[sid ^ 1] != 0 ? t.rank[sid ^ 1] : PCPPX_TCPS_NONE;
			rec.side = c.side;
			rec.flags = (uint8_t)(t.flags[sid] & 0x0F);
			o.streams[rk] = rec;
		}
	}
	const bool st = member && c.len > 0 && o.data != nullptr;
	if (__ballot(st) == 0)
		return;
	const auto [dbase, dal] = align16(o.data);  // position q (= byte position + dal) lives at dbase + q
	const auto [sbase, sal] = align16(src);     // the same for source positions (= batch offset + sal)
	// rel + len <= the side's sum: inside the stream
	copy_spans(sbase, dbase, lane, st, st ? c.off + c.pay + sal : 0ull, st ? pos + c.rel + dal : 0ull, st ? c.len : 0u,
	           s_cp[w], s_dq[w], s_sa[w]);
}
}  // namespace

uint32_t tcpstream_room(uint32_t n, uint32_t max_segments)
{
	return (max_segments == 0 || max_segments > n) ? n : max_segments;
}

uint32_t tcpstream_slots(uint32_t room)
{
	uint32_t c = kTcpsMinSlots;
	while (c < 0x80000000u && c < 2ull * room)
		c <<= 1;
	return c;
}

uint64_t tcpstream_scratch_bytes(uint32_t n, uint32_t max_segments)
{
	const uint64_t g = ((uint64_t)n + kTcpsBlockPk - 1) / kTcpsBlockPk, F = tcpstream_room(n, max_segments),
	               C = tcpstream_slots((uint32_t)F);
	return 16 + 40 * g + 4ull * n + 64 * F + 120 * C;
}

int launch_tcpstream(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0,
                     uint32_t rec_stride, const pcppx_reasm_info* info, const pcppx_tcpstream_spec* spec,
                     const pcppx_tcpstreams* out, void* scratch, hipStream_t stream)
{
	const uint32_t n = b->n, g = (uint32_t)(((uint64_t)n + kTcpsBlockPk - 1) / kTcpsBlockPk);
	const uint32_t F = tcpstream_room(n, spec->max_segments), C = tcpstream_slots(F);
	uint32_t lg = 0;
	while ((1u << lg) < C)
		++lg;
	// counters | cleared to 0: key64, segkey [C each], sum_len [2C], n_data, max_data, flags, clean [2C each] | set to all
	// ones: min_first [2C], min_fin [2C], min_rst [C] | pos [2C], rank [2C], segidx [C] | cand [F] | bbytes, base_bytes
	// [g each] | bcnt, base_cnt, four sums [g each] | rec_of [n]
	uint8_t* at = static_cast<uint8_t*>(scratch);
	Table t{};
	t.counters = reinterpret_cast<uint32_t*>(at);
	t.key64 = reinterpret_cast<unsigned long long*>(at + 16);
	t.segkey = t.key64 + C;
	t.sum_len = t.segkey + C;
	t.n_data = reinterpret_cast<uint32_t*>(t.sum_len + 2ull * C);
	t.max_data = t.n_data + 2ull * C;
	t.flags = t.max_data + 2ull * C;
	t.clean = t.flags + 2ull * C;
	uint8_t* ones = reinterpret_cast<uint8_t*>(t.clean + 2ull * C);  // at + 16 + 64 C
	t.min_first = reinterpret_cast<unsigned long long*>(ones);
	t.min_fin = reinterpret_cast<uint32_t*>(t.min_first + 2ull * C);
	t.min_rst = t.min_fin + 2ull * C;
	t.pos = reinterpret_cast<uint64_t*>(t.min_rst + C);  // at + 16 + 92 C
	t.rank = reinterpret_cast<uint32_t*>(t.pos + 2ull * C);
	t.segidx = t.rank + 2ull * C;
	t.cand = reinterpret_cast<Cand*>(t.segidx + C);  // at + 16 + 120 C
	t.room = F;
	t.slots = C;
	t.shift = 32 - lg;
	uint64_t* bbytes = reinterpret_cast<uint64_t*>(t.cand + F);
	uint64_t* base_bytes = bbytes + g;
	uint32_t* bcnt = reinterpret_cast<uint32_t*>(base_bytes + g);
	uint32_t* base_cnt = bcnt + g;
	uint32_t* bsums = base_cnt + g;  // 4 rows of g
	t.rec_of = bsums + 4ull * g;
	if (hipMemsetAsync(scratch, 0, 16 + 64ull * C, stream) != hipSuccess ||
	    hipMemsetAsync(ones, 0xFF, 28ull * C, stream) != hipSuccess)
		return PCPPX_E_HIP;
	TsIn in{ b->data, b->offsets, b->caplens, b->data_len, n, layers, ml, rec0, rec_stride, info, spec->base_clear };
	TsOut o{ out->data,       out->data_cap, out->streams,     out->disposition,
		     out->seg_stream, out->seg_pos,  out->max_streams, out->totals };
	const uint32_t gc = (F + kTcpsCandPerBlock - 1) / kTcpsCandPerBlock;
	hipLaunchKernelGGL(tcps_collect_kernel, dim3(g), dim3(kTsThreads), 0, stream, in, t);
	hipLaunchKernelGGL(tcps_second_kernel, dim3(gc), dim3(kTsThreads), 0, stream, t);
	hipLaunchKernelGGL(tcps_join_kernel, dim3(gc), dim3(kTsThreads), 0, stream, t);
	hipLaunchKernelGGL(tcps_chain_kernel, dim3(gc), dim3(kTsThreads), 0, stream, t);
	hipLaunchKernelGGL(tcps_verdict_kernel, dim3(gc), dim3(kTsThreads), 0, stream, t, in.base_clear);
	hipLaunchKernelGGL(tcps_count_kernel, dim3(g), dim3(kTsThreads), 0, stream, n, t, bbytes, bcnt, bsums);
	hipLaunchKernelGGL(tcps_base_kernel, dim3(1), dim3(64), 0, stream, g, t, bbytes, bcnt, bsums, base_bytes, base_cnt, o,
	                   spec->max_segments == 0 ? n : spec->max_segments);
	hipLaunchKernelGGL(tcps_place_kernel, dim3(g), dim3(kTsThreads), 0, stream, n, t, o, base_bytes, base_cnt);
	hipLaunchKernelGGL(tcps_emit_kernel, dim3(gc), dim3(kTsThreads), 0, stream, b->data, t, o);
	return check_launch("tcpstream", stream);
}
}  // namespace pcppx
