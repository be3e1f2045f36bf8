// pcppx_capi.cpp — the C ABI of include/pcppx.h: contexts, argument checks, kernel launches and the
// pinned, double-buffered host-to-host pipeline.
//
// One context = one GPU + one host thread (the DpdkExample-FilterTraffic model of one private worker
// per core, AppWorkerThread.h:45-162, mapped to one worker per GPU). Nothing here touches packet bytes
// on the CPU except the copy into pinned staging on the host path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "pcppx.h"
#include "pcppx_internal.h"
#include "pcppx_tlsfp.h"
#include "pcppx_dns.h"
#include "pcppx_http.h"
#include "pcppx_sip.h"
#include "pcppx_dhcp.h"
#include "pcppx_ssl.h"

namespace
{
bool ok(hipError_t e)
{
	return e == hipSuccess;
}

constexpr size_t kChunkBytes = 64u << 20;    // packet bytes per host-path chunk
constexpr uint32_t kChunkPackets = 1u << 18;  // packets per host-path chunk

struct Slot
{
	hipStream_t st = nullptr;
	hipEvent_t done = nullptr;
	uint8_t* h_data = nullptr;
	uint64_t* h_off = nullptr;
	uint32_t* h_cap = nullptr;
	pcppx_summary* h_sum = nullptr;
	pcppx_layer* h_lay = nullptr;  // FIXED rows, or (DENSE) the chunk's chains
	pcppx_brief* h_brief = nullptr;
	uint32_t* h_total = nullptr;   // DENSE: the chunk's chain entries, and the batch's up to the chunk's end
	uint8_t* d_data = nullptr;
	uint64_t* d_off = nullptr;
	uint32_t* d_cap = nullptr;
	pcppx_summary* d_sum = nullptr;
	pcppx_layer* d_lay = nullptr;
	pcppx_brief* d_brief = nullptr;
	pcppx_layer* d_dense = nullptr;  // DENSE: the chunk's chains back to back
	uint32_t* d_dsum = nullptr;      // DENSE: per-block chain totals, the chunk's total, the batch's up to the chunk's end
	hipEvent_t parsed = nullptr;     // DENSE: the chunk's chains pushed (the next chunk's positions follow them)
	uint8_t* h_match = nullptr;  // host filter path: per-packet verdicts
	uint8_t* d_match = nullptr;
	bool busy = false;
	uint32_t first = 0, count = 0, ml = 0;
	uint64_t dense_first = 0;  // DENSE: the chunk's first entry in the caller's array
	uint32_t dense_count = 0;
};

// memcpy split over persistent host threads (started with the host path, joined at pcppx_close): a single
// core copies ~8-10 GB/s, below what the PCIe link takes. The caller copies part 0 itself.
class CopyPool
{
public:
	static constexpr unsigned kThreads = 16;

	void start()
	{
		for (unsigned k = 1; k < kThreads; ++k)
			m_threads.emplace_back([this, k] { work(k); });
	}

	void stop()
	{
		{
			std::lock_guard<std::mutex> g(m_mu);
			m_quit = true;
		}
		m_cv.notify_all();
		for (auto& t : m_threads)
			t.join();
		m_threads.clear();
		m_quit = false;
	}

	// one part per >= 1 MiB, at most kThreads parts
	void copy(void* dst, const void* src, size_t bytes)
	{
		unsigned parts = (unsigned)(bytes >> 20);
		parts = parts < 1 ? 1 : (parts > kThreads ? kThreads : parts);
		if (parts == 1 || m_threads.empty())
		{
			std::memcpy(dst, src, bytes);
			return;
		}
		const size_t per = ((bytes + parts - 1) / parts + 63) & ~(size_t)63;
		{
			std::lock_guard<std::mutex> g(m_mu);
			m_dst = static_cast<uint8_t*>(dst);
			m_src = static_cast<const uint8_t*>(src);
			m_bytes = bytes;
			m_per = per;
			m_parts = parts;
			m_left = 0;
			for (unsigned k = 1; k < parts; ++k)
				m_left += k * per < bytes ? 1 : 0;
			++m_gen;
		}
		m_cv.notify_all();
		std::memcpy(dst, src, per < bytes ? per : bytes);
		std::unique_lock<std::mutex> g(m_mu);
		m_done.wait(g, [&] { return m_left == 0; });
	}

private:
	void work(unsigned k)
	{
		uint64_t seen = 0;
		for (;;)
		{
			uint8_t* d;
			const uint8_t* s;
			size_t lo, len;
			{
				std::unique_lock<std::mutex> g(m_mu);
				m_cv.wait(g, [&] { return m_quit || m_gen != seen; });
				if (m_quit)
					return;
				seen = m_gen;
				lo = k * m_per;
				if (k >= m_parts || lo >= m_bytes)
					continue;
				len = m_bytes - lo < m_per ? m_bytes - lo : m_per;
				d = m_dst + lo;
				s = m_src + lo;
			}
			std::memcpy(d, s, len);
			{
				std::lock_guard<std::mutex> g(m_mu);
				--m_left;
			}
			m_done.notify_one();
		}
	}

	std::vector<std::thread> m_threads;
	std::mutex m_mu;
	std::condition_variable m_cv, m_done;
	uint8_t* m_dst = nullptr;
	const uint8_t* m_src = nullptr;
	size_t m_bytes = 0, m_per = 0;
	unsigned m_parts = 0, m_left = 0;
	uint64_t m_gen = 0;
	bool m_quit = false;
};

constexpr uint32_t kDefaultFlowSlots = 1u << 22;  // 64 MiB of flow table in HBM
constexpr uint32_t kMaxSlots = 3;                   // host-path chunk slots in flight

// Stream-ordered scratch owned by a context and shared by its calls, with an event after each call's last kernel: the
// next call (on whatever stream) waits for it on its own stream before touching the scratch, and a larger size is
// reallocated in stream order behind that wait -- calls on one context are ordered even across streams, and no call
// stalls the device or another stream.
struct Scratch
{
	void* ptr = nullptr;
	uint64_t bytes = 0;
	hipEvent_t done = nullptr;
	bool pending = false;

	// at least `want` bytes for work on st, behind the previous user
	int acquire(hipStream_t st, uint64_t want)
	{
		if (done == nullptr && !ok(hipEventCreateWithFlags(&done, hipEventDisableTiming)))
			return PCPPX_E_HIP;
		if (pending && !ok(hipStreamWaitEvent(st, done, 0)))
			return PCPPX_E_HIP;
		if (bytes < want)
		{
			if (ptr != nullptr && !ok(hipFreeAsync(ptr, st)))
				return PCPPX_E_HIP;
			ptr = nullptr;
			bytes = 0;
			if (!ok(hipMallocAsync(&ptr, want, st)))
				return PCPPX_E_NOMEM;
			bytes = want;
		}
		return PCPPX_OK;
	}
	// after the call's last kernel on st
	int mark_used(hipStream_t st)
	{
		if (!ok(hipEventRecord(done, st)))
			return PCPPX_E_HIP;
		pending = true;
		return PCPPX_OK;
	}
	// teardown, in this order: the last user is done; the memory goes back on st; the event goes
	void wait() const
	{
		if (pending)
			(void)hipEventSynchronize(done);
	}
	void release(hipStream_t st) const
	{
		if (ptr)
			(void)hipFreeAsync(ptr, st);
	}
	void destroy_event() const
	{
		if (done)
			(void)hipEventDestroy(done);
	}
};
}  // namespace

struct pcppx_ctx
{
	int device = 0;
	hipStream_t stream = nullptr;
	bool host_ready = false;
	Slot slots[kMaxSlots];
	uint32_t nslots = 0;  // slots allocated and used by the host paths
	CopyPool copier;      // staging and drain copies of the host paths
	// host filter path (pcppx_filter_reset / pcppx_filter_batch_host): the worker's flow table in HBM
	uint64_t* d_keys = nullptr;
	uint64_t* d_first = nullptr;
	pcppx_packet_stats* d_stats = nullptr;
	uint32_t flow_slots = 0;
	uint64_t seq = 0;
	// pcppx_flow_count_device: the partitioned flush's record queues (16-B records) and, allocated apart, the queue
	// lengths (zero between calls)
	Scratch flow;
	uint32_t* d_flow_fill = nullptr;
	// pcppx_records.proto_stats: the parse's per-wave collectStats records (16 B per 64 packets), summed into the
	// caller's counters by a second kernel
	Scratch stats;
	// pcppx_select_device: the per-block sums and bases (28 B per kSelectBlockPk packets)
	Scratch select;
	// pcppx_steer_device: the block sums per bucket and the bucket totals (steer_scratch_bytes)
	Scratch steer;
	// pcppx_defrag_device: the group table, the candidate records and the block sums (defrag_scratch_bytes)
	Scratch defrag;
	// pcppx_tcpstream_device: the connection and segment tables, the candidate records, the per-packet words and the
	// block sums (tcpstream_scratch_bytes)
	Scratch tcpstream;
	// pcppx_frag_device: the block sums and bases and the per-packet plans (frag_scratch_bytes)
	Scratch frag;
	// pcppx_tlsfp_device, pcppx_dns_device, pcppx_http_device, pcppx_ssl_device, pcppx_sip_device, pcppx_dhcp_device:
	// each one's per-packet plans and block sums and bases (<op>_scratch_bytes)
	Scratch tlsfp, dns, http, ssl, sip, dhcp;
	// the engine's header-window choice for PCPPX_WINDOW_DEFAULT launches: a sampled parse (every launch until the first
	// decision, then one in kWinEvery) first adds the live packets and deep stacks of about 64 of its tiles to d_win (never
	// cleared); after it, a private stream copies the counters into a page-locked mirror, which a later launch reads once
	// the copy is done (no wait on any stream)
	unsigned long long* d_win = nullptr;
	unsigned long long* h_win = nullptr;
	hipStream_t win_stream = nullptr;
	hipEvent_t win_parsed = nullptr, win_copied = nullptr;
	bool win_ready = false, win_pending = false;
	unsigned long long win_live = 0, win_deep = 0;  // the mirror at the last decision
	int deep_traffic = -1;                            // -1: not known yet; 0: plain stacks; 1: deep stacks
	uint64_t win_launches = 0;                        // DEFAULT-window parses so far (the sampling schedule)
};

namespace
{
// ---- the engine's header window (PCPPX_WINDOW_DEFAULT) ----
constexpr unsigned long long kWinMinSample = 2048;  // sampled packets per decision (a launch samples up to ~4096)
constexpr unsigned long long kWinDeepShare = 256;   // deep stacks above 1 in 256 sampled packets: deep traffic
constexpr uint64_t kWinEvery = 16;                  // once decided, one parse in 16 is sampled (the traffic may change)

bool ensure_win(pcppx_ctx* c)
{
	if (c->win_ready)
		return true;
	const bool good = ok(hipMalloc(reinterpret_cast<void**>(&c->d_win), 2 * sizeof(unsigned long long))) &&
	                  ok(hipMemset(c->d_win, 0, 2 * sizeof(unsigned long long))) &&
	                  ok(hipHostMalloc(reinterpret_cast<void**>(&c->h_win), 2 * sizeof(unsigned long long))) &&
	                  ok(hipStreamCreateWithFlags(&c->win_stream, hipStreamNonBlocking)) &&
	                  ok(hipEventCreateWithFlags(&c->win_parsed, hipEventDisableTiming)) &&
	                  ok(hipEventCreateWithFlags(&c->win_copied, hipEventDisableTiming));
	if (!good)
	{
		(void)hipGetLastError();
		return false;
	}
	c->h_win[0] = c->h_win[1] = 0;
	c->win_ready = true;
	return true;
}

// fold a finished counter copy into the decision (wait: block until the copy in flight is done)
void update_window(pcppx_ctx* c, bool wait)
{
	if (!c->win_pending)
		return;
	if (wait ? !ok(hipEventSynchronize(c->win_copied)) : hipEventQuery(c->win_copied) != hipSuccess)
		return;
	c->win_pending = false;
	const unsigned long long live = c->h_win[0] - c->win_live, deep = c->h_win[1] - c->win_deep;
	if (live < kWinMinSample)
		return;
	c->deep_traffic = deep * kWinDeepShare > live ? 1 : 0;
	c->win_live = c->h_win[0];
	c->win_deep = c->h_win[1];
}

// the window a launch runs with: an explicit DEEP / SHORT as asked; DEFAULT follows the traffic this context has seen
// (deep stacks: the two-round window for checksum launches too; plain stacks: one round for parse-only launches too).
// The records are the same whichever window runs.
pcppx_opts resolve_window(pcppx_ctx* c, const pcppx_opts* o)
{
	pcppx_opts e = *o;
	if (o->window != PCPPX_WINDOW_DEFAULT)
		return e;
	update_window(c, false);
	if (c->deep_traffic == 1 && o->want_checksums)
		e.window = PCPPX_WINDOW_DEEP;
	else if (c->deep_traffic == 0 && !o->want_checksums)
		e.window = PCPPX_WINDOW_SHORT;
	return e;
}

// the counters a parse samples into, or null: a PCPPX_WINDOW_DEFAULT parse every time until the first decision, then
// one in kWinEvery; a parse whose window the caller forced never (the choice follows the DEFAULT parses' traffic)
unsigned long long* window_sample(pcppx_ctx* c, const pcppx_opts* o)
{
	if (o->window != PCPPX_WINDOW_DEFAULT || !ensure_win(c))
		return nullptr;
	update_window(c, false);
	const uint64_t k = c->win_launches++;
	return (c->deep_traffic < 0 || k % kWinEvery == 0) ? c->d_win : nullptr;
}

// after a sampled parse on st (win: window_sample's counters): copy the counters out behind it on the private stream
// (one copy in flight)
void note_window(pcppx_ctx* c, hipStream_t st, const unsigned long long* win)
{
	if (win == nullptr || !c->win_ready || c->win_pending)
		return;
	if (ok(hipEventRecord(c->win_parsed, st)) && ok(hipStreamWaitEvent(c->win_stream, c->win_parsed, 0)) &&
	    ok(hipMemcpyAsync(c->h_win, c->d_win, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->win_stream)) &&
	    ok(hipEventRecord(c->win_copied, c->win_stream)))
		c->win_pending = true;
	else
		(void)hipGetLastError();
}

int valid_opts(const pcppx_opts* o)
{
	if (o == nullptr || o->max_layers > PCPPX_MAX_LAYERS || o->window > PCPPX_WINDOW_SHORT ||
	    o->layout > PCPPX_LAYOUT_DENSE || (o->layout == PCPPX_LAYOUT_PACKED && o->max_layers > PCPPX_PACKED_MAX_LAYERS))
		return PCPPX_E_INVAL;
	return PCPPX_OK;
}

// the device path's record arguments: layers when max_layers > 0; a summary unless the caller wants only the
// summary-free outputs -- the 5-tuple extract, the dense flow-key column and / or the collectStats counters (a
// FilterTraffic-style consumer reads nothing else) -- with no layers (a PACKED layout is decoded through the summary's
// n_layers)
bool valid_device_records(const pcppx_opts* o, const pcppx_records* r)
{
	if (o->max_layers != 0 && r->layers == nullptr)
		return false;
	if (r->summary == nullptr && r->brief == nullptr &&
	    (o->max_layers != 0 || (r->tuples == nullptr && r->flow_keys == nullptr && r->proto_stats == nullptr)))
		return false;
	return o->layout != PCPPX_LAYOUT_DENSE;  // DENSE: the host path's layout
}

// launch a device parse (plain or with the fused reassembly output) with the collectStats reduction when
// r->proto_stats is set
int device_parse(pcppx_ctx* c, const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r, pcppx_reasm_info* info,
                 hipStream_t st)
{
	void* ws = nullptr;
	if (r->proto_stats != nullptr)
	{
		const int rc = c->stats.acquire(st, (uint64_t)pcppx::parse_waves(b->n) * 16);
		if (rc != PCPPX_OK)
			return rc;
		ws = c->stats.ptr;
	}
	const pcppx_opts eo = resolve_window(c, o);
	unsigned long long* win = window_sample(c, o);
	int rc = info ? pcppx::launch_parse_reasm(b, &eo, r, info, st, ws, win) : pcppx::launch_parse(b, &eo, r, st, ws, win);
	if (rc == PCPPX_OK)
		note_window(c, st, win);
	if (rc != PCPPX_OK || ws == nullptr)
		return rc;
	rc = pcppx::launch_proto_stats_reduce(ws, b->n, r->proto_stats, st);
	return rc != PCPPX_OK ? rc : c->stats.mark_used(st);
}

void free_slot(Slot& s)
{
	if (s.st) (void)hipStreamDestroy(s.st);
	if (s.done) (void)hipEventDestroy(s.done);
	if (s.parsed) (void)hipEventDestroy(s.parsed);
	(void)hipHostFree(s.h_brief);
	(void)hipHostFree(s.h_total);
	(void)hipFree(s.d_brief);
	(void)hipFree(s.d_dense);
	(void)hipFree(s.d_dsum);
	(void)hipHostFree(s.h_data);
	(void)hipHostFree(s.h_off);
	(void)hipHostFree(s.h_cap);
	(void)hipHostFree(s.h_sum);
	(void)hipHostFree(s.h_lay);
	(void)hipFree(s.d_data);
	(void)hipFree(s.d_off);
	(void)hipFree(s.d_cap);
	(void)hipFree(s.d_sum);
	(void)hipFree(s.d_lay);
	(void)hipHostFree(s.h_match);
	(void)hipFree(s.d_match);
	s = Slot();
}

int init_host_path(pcppx_ctx* c)
{
	if (c->host_ready)
		return PCPPX_OK;
	// three slots: the H2D copy of chunk k+1 overlaps the kernel of chunk k and the drain of chunk k-1
	c->nslots = kMaxSlots;
	for (uint32_t si = 0; si < c->nslots; ++si)
	{
		Slot& s = c->slots[si];
		bool good = ok(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking)) && ok(hipEventCreate(&s.done)) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_data), kChunkBytes + 16)) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_off), kChunkPackets * sizeof(uint64_t))) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_cap), kChunkPackets * sizeof(uint32_t))) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_sum), kChunkPackets * sizeof(pcppx_summary))) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_lay),
		                             (size_t)kChunkPackets * PCPPX_MAX_LAYERS * sizeof(pcppx_layer))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_data), kChunkBytes + 16)) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_off), kChunkPackets * sizeof(uint64_t))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_cap), kChunkPackets * sizeof(uint32_t))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_sum), kChunkPackets * sizeof(pcppx_summary))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_lay),
		                         (size_t)kChunkPackets * PCPPX_MAX_LAYERS * sizeof(pcppx_layer))) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_match), kChunkPackets)) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_match), kChunkPackets)) &&
		            ok(hipEventCreateWithFlags(&s.parsed, hipEventDisableTiming)) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_brief), kChunkPackets * sizeof(pcppx_brief))) &&
		            ok(hipHostMalloc(reinterpret_cast<void**>(&s.h_total), 2 * sizeof(uint32_t))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_brief), kChunkPackets * sizeof(pcppx_brief))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_dense),
		                         (size_t)kChunkPackets * PCPPX_MAX_LAYERS * sizeof(pcppx_layer))) &&
		            ok(hipMalloc(reinterpret_cast<void**>(&s.d_dsum),
		                         (pcppx::dense_blocks(kChunkPackets) + 2) * sizeof(uint32_t)));
		if (!good)
		{
			for (Slot& t : c->slots)
				free_slot(t);
			return PCPPX_E_NOMEM;
		}
	}
	c->copier.start();
	c->host_ready = true;
	return PCPPX_OK;
}

// true if p is page-locked host memory the GPU can DMA from directly
bool is_pinned(const void* p)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess)
	{
		(void)hipGetLastError();  // pageable memory: clear the error so launch checks do not see it
		return false;
	}
	return a.type == hipMemoryTypeHost;
}

// the device mapping of page-locked host memory (kernels store into it directly), or null
void* mapped(void* p)
{
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess || a.type != hipMemoryTypeHost || a.devicePointer == nullptr)
	{
		(void)hipGetLastError();
		return nullptr;
	}
	return a.devicePointer;
}

// Packets [i, j) of a host batch as one byte range [*base, *base + *bytes): ascending, each starting at most kMaxGap
// bytes after the previous one ends (packed batches; a memory-mapped capture's packets with their record headers
// between them, pcppx_pcap_map_batch): returns j, or i if packet i does not start such a run.
constexpr uint64_t kMaxGap = 256;
uint32_t contiguous_chunk(const pcppx_batch* b, uint32_t i, uint64_t* base, size_t* bytes)
{
	uint64_t end = b->offsets[i];
	*base = end;
	uint32_t j = i;
	while (j < b->n && j - i < kChunkPackets)
	{
		const uint64_t off = b->offsets[j];
		const uint32_t cap = b->caplens[j];
		if (off < end || off - end > kMaxGap || off + cap > b->data_len || off + cap < off)
			break;
		if (off + cap - *base > kChunkBytes)
			break;
		end = off + cap;
		++j;
	}
	*bytes = (size_t)(end - *base);
	return j;
}
constexpr uint32_t kMinRun = 4096;  // a shorter run that stops at a discontinuity is gathered per packet instead

// gather packets [i, j) of a host batch into the slot's pinned staging, rebasing offsets; returns j.
// Contiguous runs are not staged: *direct is then the source of the H2D copy, page-locked or not (the runtime DMAs a
// pageable range as fast as a page-locked one, 56 GB/s from a file map, profiles/r04f_h2d_probe.txt, where a copy
// into staging first ran at 30 GB/s per thread); scattered packets are gathered into the staging.
// *pos_out: the bytes to copy to the device; *len_out: the chunk's data_len there, which is larger only when a gathered
// chunk holds an oversize packet (no byte of it is staged, but its descriptor must stay in bounds).
uint32_t stage_chunk(Slot& s, const pcppx_batch* b, uint32_t i, size_t* pos_out, uint64_t* len_out,
                     const uint8_t** direct)
{
	*direct = nullptr;
	{
		uint64_t base = 0;
		size_t bytes = 0;
		const uint32_t j = contiguous_chunk(b, i, &base, &bytes);
		// a run that ends the batch, a long run, or one that stops only because the next packet (ascending) would not fit
		// the chunk: copied straight from the caller's bytes. (A next packet below the run -- an unordered batch -- is
		// no such reason: its offset minus the run's base would wrap.)
		if (j > i && (j == b->n || j - i >= kMinRun ||
		              (b->offsets[j] >= base && b->offsets[j] + b->caplens[j] - base > kChunkBytes)))
		{
			for (uint32_t k = i; k < j; ++k)
			{
				s.h_off[k - i] = b->offsets[k] - base;
				s.h_cap[k - i] = b->caplens[k];
			}
			*direct = b->data + base;
			*pos_out = bytes;
			*len_out = bytes;
			return j;
		}
	}
	size_t pos = 0;
	uint64_t oversize = 0;  // the largest in-bounds caplen above PCPPX_MAX_CAPLEN
	uint32_t j = i;
	while (j < b->n && j - i < kChunkPackets)
	{
		const uint64_t off = b->offsets[j];
		const uint32_t cap = b->caplens[j];
		const bool in_bounds = off + cap <= b->data_len && off + cap >= off;
		// the kernels read the bytes of no other packet (desc_flags: PCPPX_F_BAD_DESC, PCPPX_F_OVERSIZE)
		const bool parsed = in_bounds && cap <= PCPPX_MAX_CAPLEN;
		const size_t take = parsed ? cap : 0;
		if (pos + take > kChunkBytes && j > i)
			break;
		if (parsed)
		{
			std::memcpy(s.h_data + pos, b->data + off, cap);
			s.h_off[j - i] = pos;
			pos += cap;
		}
		else if (in_bounds)
		{
			s.h_off[j - i] = 0;  // kernel flags PCPPX_F_OVERSIZE, as the device path does: no bytes staged
			oversize = cap > oversize ? cap : oversize;
		}
		else
			s.h_off[j - i] = ~0ull >> 1;  // kernel flags PCPPX_F_BAD_DESC
		s.h_cap[j - i] = cap;
		++j;
	}
	*pos_out = pos;
	*len_out = pos > oversize ? pos : oversize;
	return j;
}

bool upload_chunk(Slot& s, size_t pos, uint32_t cnt, const uint8_t* direct = nullptr)
{
	// a chunk of zero bytes copies one placeholder byte, from the slot's own staging: a direct run of empty packets may
	// start at the very end of the caller's buffer
	return ok(hipMemcpyAsync(s.d_data, direct && pos ? direct : s.h_data, pos ? pos : 1, hipMemcpyHostToDevice, s.st)) &&
	       ok(hipMemcpyAsync(s.d_off, s.h_off, cnt * sizeof(uint64_t), hipMemcpyHostToDevice, s.st)) &&
	       ok(hipMemcpyAsync(s.d_cap, s.h_cap, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s.st));
}

void free_filter(pcppx_ctx* c)
{
	(void)hipFree(c->d_keys);
	(void)hipFree(c->d_first);
	(void)hipFree(c->d_stats);
	c->d_keys = c->d_first = nullptr;
	c->d_stats = nullptr;
	c->flow_slots = 0;
	c->seq = 0;
}

int flow_count(pcppx_ctx* c, const pcppx_summary* summary, const uint32_t* keys_in, const uint32_t* caplens, uint32_t n,
               uint32_t* keys, uint64_t* packets, uint64_t* bytes, uint32_t capacity, uint64_t* stats, void* hip_stream);

// forget every slot's chunk without copying it out: after an error mid-call, and at the start of each host
// call, so that a later call never drains a stale chunk into its own (possibly smaller) output arrays
void abandon_slots(pcppx_ctx* c)
{
	for (Slot& s : c->slots)
	{
		if (s.st)
			(void)hipStreamSynchronize(s.st);
		s.busy = false;
	}
	(void)hipGetLastError();
}

// copy a finished chunk's records from pinned memory to the caller's arrays (nothing to copy when the
// caller's arrays are pinned: the chunk's D2H wrote them directly)
// (dense_direct: the DENSE chains were pushed into the caller's array through its device mapping; otherwise they sit in
// the slot's staging buffer -- a pinned caller array without a device mapping takes this path too)
void drain(CopyPool& cp, Slot& s, pcppx_records* out, bool direct_out, bool dense, bool dense_direct, uint64_t* written)
{
	if (dense && s.ml && out->layers)  // the chunk's chains: [batch total up to its end - its own, batch total)
	{
		s.dense_count = s.h_total[0];
		s.dense_first = s.h_total[1] - s.h_total[0];
		*written = s.h_total[1] > *written ? s.h_total[1] : *written;
	}
	if (!direct_out)
	{
		if (out->summary)
			cp.copy(out->summary + s.first, s.h_sum, (size_t)s.count * sizeof(pcppx_summary));
		if (out->brief)
			cp.copy(out->brief + s.first, s.h_brief, (size_t)s.count * sizeof(pcppx_brief));
		if (s.ml && out->layers && !dense)
			cp.copy(out->layers + (size_t)s.first * s.ml, s.h_lay, (size_t)s.count * s.ml * sizeof(pcppx_layer));
	}
	if (s.ml && out->layers && dense && !dense_direct)
		cp.copy(out->layers + s.dense_first, s.h_lay, (size_t)s.dense_count * sizeof(pcppx_layer));
	if (out->flow_keys)  // the dense hash5 column, from the host copy of the summaries / briefs
		for (uint32_t k = 0; k < s.count; ++k)
			out->flow_keys[s.first + k] = out->summary ? out->summary[s.first + k].hash5 : out->brief[s.first + k].hash5;
	s.busy = false;
}

// pcppx_parse_batch_host's chunk pipeline (argument checks done; slots idle on entry)
int parse_host_run(pcppx_ctx* c, const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r)
{
	int rc = PCPPX_OK;
	const uint32_t ml = o->max_layers;
	const bool rows = ml != 0 && r->layers != nullptr;
	const bool dense = rows && o->layout == PCPPX_LAYOUT_DENSE;
	// a NIC ring / pcppx_host_alloc result buffer: records come back by DMA straight into the caller's arrays
	const bool direct_out = (r->summary == nullptr || is_pinned(r->summary)) &&
	                        (r->brief == nullptr || is_pinned(r->brief)) && (!rows || is_pinned(r->layers));
	uint64_t written = 0;
	// DENSE: the chains are pushed by a kernel through the device mapping of page-locked memory (the caller's array, or
	// the slot's staging buffer), their positions chained on the device chunk after chunk -- no host round trip to learn
	// a chunk's count before its copy
	const uint32_t kTot = pcppx::dense_blocks(kChunkPackets);  // d_dsum[kTot]: the chunk's, [kTot + 1]: cumulative
	// a page-locked caller array without a device mapping (pinned by another runtime, say) is still filled: its chains
	// are staged like a pageable array's (the FIXED rows reach such an array by DMA)
	pcppx_layer* lay_map = dense && direct_out ? static_cast<pcppx_layer*>(mapped(r->layers)) : nullptr;
	const bool dense_direct = lay_map != nullptr;
	Slot* prev = nullptr;  // DENSE: the previous chunk (its cumulative count is this chunk's base)
	uint32_t i = 0, k = 0;
	while (i < b->n)
	{
		Slot& s = c->slots[k % c->nslots];
		if (s.busy)
		{
			if (!ok(hipEventSynchronize(s.done)))
				return PCPPX_E_HIP;
			drain(c->copier, s, r, direct_out, dense, dense_direct, &written);
		}
		size_t pos = 0;
		uint64_t len = 0;
		const uint8_t* direct = nullptr;
		const uint32_t j = stage_chunk(s, b, i, &pos, &len, &direct);
		const uint32_t cnt = j - i;
		if (!upload_chunk(s, pos, cnt, direct))
			return PCPPX_E_HIP;
		pcppx_batch db{ s.d_data, s.d_off, s.d_cap, len, cnt, b->linktype, 0 };
		pcppx_records dr{};
		dr.summary = r->summary ? s.d_sum : nullptr;
		dr.brief = r->brief ? s.d_brief : nullptr;
		dr.layers = ml ? s.d_lay : nullptr;
		pcppx_opts fo = resolve_window(c, o);
		fo.layout = PCPPX_LAYOUT_FIXED;  // DENSE is compacted from the chunk's FIXED rows below
		unsigned long long* win = window_sample(c, o);
		rc = pcppx::launch_parse(&db, &fo, &dr, s.st, nullptr, win);
		if (rc == PCPPX_OK)
			note_window(c, s.st, win);
		if (rc == PCPPX_OK && dense)
			rc = pcppx::launch_dense_compact(s.d_lay,
			                                 dr.brief ? reinterpret_cast<const uint8_t*>(s.d_brief) + 14
			                                          : reinterpret_cast<const uint8_t*>(s.d_sum) + 14,
			                                 dr.brief ? sizeof(pcppx_brief) : sizeof(pcppx_summary), cnt, ml, s.d_dense,
			                                 s.d_dsum, s.d_dsum + pcppx::dense_blocks(kChunkPackets), s.st);
		if (rc != PCPPX_OK)
			return rc;
		pcppx_summary* hs = direct_out && r->summary ? r->summary + i : s.h_sum;
		pcppx_brief* hb = direct_out && r->brief ? r->brief + i : s.h_brief;
		pcppx_layer* hl = direct_out && rows ? r->layers + (size_t)i * ml : s.h_lay;
		bool good = (!r->summary ||
		             ok(hipMemcpyAsync(hs, s.d_sum, cnt * sizeof(pcppx_summary), hipMemcpyDeviceToHost, s.st))) &&
		            (!r->brief || ok(hipMemcpyAsync(hb, s.d_brief, cnt * sizeof(pcppx_brief), hipMemcpyDeviceToHost, s.st)));
		if (dense)
		{
			pcppx_layer* to = dense_direct ? lay_map : static_cast<pcppx_layer*>(mapped(s.h_lay));
			good = good && to != nullptr && (prev == nullptr || ok(hipStreamWaitEvent(s.st, prev->parsed, 0))) &&
			       pcppx::launch_dense_push(s.d_dense, s.d_dsum + kTot, prev ? prev->d_dsum + kTot + 1 : nullptr, to,
			                                dense_direct, s.d_dsum + kTot + 1, s.st) == PCPPX_OK &&
			       ok(hipEventRecord(s.parsed, s.st)) &&
			       ok(hipMemcpyAsync(s.h_total, s.d_dsum + kTot, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s.st)) &&
			       ok(hipEventRecord(s.done, s.st));
			prev = &s;
		}
		else
			good = good &&
			       (!rows ||
			        ok(hipMemcpyAsync(hl, s.d_lay, (size_t)cnt * ml * sizeof(pcppx_layer), hipMemcpyDeviceToHost, s.st))) &&
			       ok(hipEventRecord(s.done, s.st));
		if (!good)
			return PCPPX_E_HIP;
		s.busy = true;
		s.first = i;
		s.count = cnt;
		s.ml = ml;
		i = j;
		++k;
	}
	for (Slot& s : c->slots)
		if (s.busy)
		{
			if (!ok(hipEventSynchronize(s.done)))
				return PCPPX_E_HIP;
			drain(c->copier, s, r, direct_out, dense, dense_direct, &written);
		}
	r->layers_written = dense ? written : (rows ? (uint64_t)b->n * ml : 0);
	return PCPPX_OK;
}

// pcppx_filter_batch_host's chunk pipeline (argument checks done; slots idle on entry)
int filter_host_run(pcppx_ctx* c, const pcppx_batch* b, const pcppx_match_spec* spec, uint8_t* matched,
                    pcppx_packet_stats* stats)
{
	int rc = PCPPX_OK;
	pcppx_opts o;
	pcppx_default_opts(&o);
	o.want_checksums = 0;  // the worker reads addresses, ports and the protocol mask only
	const uint32_t ml = o.max_layers;
	uint32_t i = 0, k = 0;
	Slot* prev = nullptr;
	while (i < b->n)
	{
		Slot& s = c->slots[k % c->nslots];
		if (s.busy)
		{
			if (!ok(hipEventSynchronize(s.done)))
				return PCPPX_E_HIP;
			std::memcpy(matched + s.first, s.h_match, s.count);
			s.busy = false;
		}
		size_t pos = 0;
		uint64_t len = 0;
		const uint8_t* direct = nullptr;
		const uint32_t j = stage_chunk(s, b, i, &pos, &len, &direct);
		const uint32_t cnt = j - i;
		if (!upload_chunk(s, pos, cnt, direct))
			return PCPPX_E_HIP;
		// the flow table is shared by consecutive chunks: chunk k's lookups run after chunk k-1's marks
		if (prev != nullptr && !ok(hipStreamWaitEvent(s.st, prev->done, 0)))
			return PCPPX_E_HIP;
		pcppx_batch db{ s.d_data, s.d_off, s.d_cap, len, cnt, b->linktype, 0 };
		pcppx_records dr{};
		dr.summary = s.d_sum;
		dr.layers = s.d_lay;
		const pcppx_opts eo = resolve_window(c, &o);
		unsigned long long* win = window_sample(c, &o);
		rc = pcppx::launch_parse(&db, &eo, &dr, s.st, nullptr, win);
		if (rc == PCPPX_OK)
			note_window(c, s.st, win);
		if (rc == PCPPX_OK)
			rc = pcppx::launch_filter(&db, &dr, ml, spec, c->seq + i, c->d_keys, c->d_first, c->flow_slots,
			                          s.d_match, c->d_stats, s.st);
		if (rc != PCPPX_OK)
			return rc;
		if (!ok(hipMemcpyAsync(s.h_match, s.d_match, cnt, hipMemcpyDeviceToHost, s.st)) ||
		    !ok(hipEventRecord(s.done, s.st)))
			return PCPPX_E_HIP;
		s.busy = true;
		s.first = i;
		s.count = cnt;
		prev = &s;
		i = j;
		++k;
	}
	for (Slot& s : c->slots)
		if (s.busy)
		{
			if (!ok(hipEventSynchronize(s.done)))
				return PCPPX_E_HIP;
			std::memcpy(matched + s.first, s.h_match, s.count);
			s.busy = false;
		}
	c->seq += b->n;
	if (stats != nullptr &&
	    (!ok(hipMemcpy(stats, c->d_stats, sizeof(pcppx_packet_stats), hipMemcpyDeviceToHost))))
		return PCPPX_E_HIP;
	return PCPPX_OK;
}
}  // namespace

extern "C"
{
	int pcppx_abi_version(void)
	{
		return PCPPX_ABI_VERSION;
	}

	const char* pcppx_strerror(int err)
	{
		switch (err)
		{
		case PCPPX_OK: return "ok";
		case PCPPX_E_INVAL: return "invalid argument";
		case PCPPX_E_NODEV: return "no such HIP device";
		case PCPPX_E_HIP: return "HIP runtime error";
		case PCPPX_E_NOMEM: return "out of device or pinned memory";
		case PCPPX_E_LINKTYPE: return "link type not handled";
		default: return "unknown error";
		}
	}

	int pcppx_runtime_info(int device, char* buf, size_t len)
	{
		if (buf == nullptr || len == 0)
			return PCPPX_E_INVAL;
		int rt = 0, drv = 0;
		(void)hipRuntimeGetVersion(&rt);
		(void)hipDriverGetVersion(&drv);
		hipDeviceProp_t prop;
		if (!ok(hipGetDeviceProperties(&prop, device)))
		{
			snprintf(buf, len, "hip runtime %d driver %d, device %d unavailable", rt, drv, device);
			return PCPPX_E_NODEV;
		}
		snprintf(buf, len, "hip runtime %d driver %d, device %d: %s (%s), %d CUs, %.1f GiB", rt, drv, device,
		         prop.name, prop.gcnArchName, prop.multiProcessorCount,
		         (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0));
		return PCPPX_OK;
	}

	int pcppx_device_count(int* out)
	{
		if (out == nullptr)
			return PCPPX_E_INVAL;
		int n = 0;
		if (!ok(hipGetDeviceCount(&n)))
			n = 0;
		*out = n;
		return PCPPX_OK;
	}

	void pcppx_default_opts(pcppx_opts* o)
	{
		if (o == nullptr)
			return;
		o->parse_until_family = 0;  // UnknownProtocol
		o->parse_until_osi = 8;     // OsiModelLayerUnknown
		o->want_checksums = 1;
		o->max_layers = PCPPX_MAX_LAYERS;
		o->window = PCPPX_WINDOW_DEFAULT;
		o->layout = PCPPX_LAYOUT_FIXED;
		o->reserved[0] = o->reserved[1] = o->reserved[2] = 0;
	}

	int pcppx_open(int device, pcppx_ctx** out)
	{
		if (out == nullptr)
			return PCPPX_E_INVAL;
		*out = nullptr;
		int n = 0;
		if (!ok(hipGetDeviceCount(&n)) || device < 0 || device >= n)
			return PCPPX_E_NODEV;
		if (!ok(hipSetDevice(device)))
			return PCPPX_E_HIP;
		pcppx_ctx* c = new (std::nothrow) pcppx_ctx();
		if (c == nullptr)
			return PCPPX_E_NOMEM;
		c->device = device;
		if (!ok(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)))
		{
			delete c;
			return PCPPX_E_HIP;
		}
		*out = c;
		return PCPPX_OK;
	}

	void pcppx_close(pcppx_ctx* c)
	{
		if (c == nullptr)
			return;
		(void)hipSetDevice(c->device);
		(void)hipStreamSynchronize(c->stream);
		if (c->host_ready)
			c->copier.stop();
		for (Slot& s : c->slots)
		{
			if (s.st)
				(void)hipStreamSynchronize(s.st);
			free_slot(s);
		}
		free_filter(c);
		// the scratch is stream-ordered memory (hipMallocAsync): released on the context's stream
		c->flow.wait();
		c->stats.wait();
		c->flow.release(c->stream);
		if (c->d_flow_fill)
			(void)hipFreeAsync(c->d_flow_fill, c->stream);
		c->stats.release(c->stream);
		c->select.wait();
		c->select.release(c->stream);
		c->steer.wait();
		c->steer.release(c->stream);
		c->defrag.wait();
		c->defrag.release(c->stream);
		c->tcpstream.wait();
		c->tcpstream.release(c->stream);
		c->frag.wait();
		c->frag.release(c->stream);
		c->tlsfp.wait();
		c->tlsfp.release(c->stream);
		c->dns.wait();
		c->dns.release(c->stream);
		c->http.wait();
		c->http.release(c->stream);
		c->ssl.wait();
		c->ssl.release(c->stream);
		c->sip.wait();
		c->sip.release(c->stream);
		c->dhcp.wait();
		c->dhcp.release(c->stream);
		(void)hipStreamSynchronize(c->stream);
		if (c->win_ready)
		{
			(void)hipStreamSynchronize(c->win_stream);
			(void)hipStreamDestroy(c->win_stream);
			(void)hipEventDestroy(c->win_parsed);
			(void)hipEventDestroy(c->win_copied);
			(void)hipFree(c->d_win);
			(void)hipHostFree(c->h_win);
		}
		for (const Scratch* x : { &c->flow, &c->stats, &c->select, &c->steer, &c->defrag, &c->tcpstream, &c->frag,
		                         &c->tlsfp, &c->dns, &c->http, &c->ssl, &c->sip, &c->dhcp })
			x->destroy_event();
		(void)hipStreamDestroy(c->stream);
		delete c;
	}

	int pcppx_window_choice(pcppx_ctx* c, int want_checksums, int* window)
	{
		if (c == nullptr || window == nullptr)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		update_window(c, true);
		pcppx_opts o;
		pcppx_default_opts(&o);
		o.want_checksums = want_checksums ? 1 : 0;
		*window = resolve_window(c, &o).window;
		return PCPPX_OK;
	}

	void* pcppx_ctx_stream(pcppx_ctx* c)
	{
		return c ? static_cast<void*>(c->stream) : nullptr;
	}

	int pcppx_sync(pcppx_ctx* c)
	{
		if (c == nullptr)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)) || !ok(hipStreamSynchronize(c->stream)))
			return PCPPX_E_HIP;
		return PCPPX_OK;
	}

	int pcppx_parse_batch_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r,
	                             void* hip_stream)
	{
		if (c == nullptr || b == nullptr || r == nullptr || valid_opts(o) != PCPPX_OK)
			return PCPPX_E_INVAL;
		r->layout = o->layout;  // set for an empty batch too: a reused records struct keeps no stale count
		r->layers_written = 0;
		if (b->n == 0)
			return PCPPX_OK;
		if (b->data == nullptr || b->offsets == nullptr || b->caplens == nullptr || !valid_device_records(o, r))
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		r->layers_written = o->max_layers ? (uint64_t)b->n * o->max_layers : 0;
		return device_parse(c, b, o, r, nullptr, static_cast<hipStream_t>(hip_stream));
	}

	int pcppx_parse_batch_host(pcppx_ctx* c, const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r)
	{
		if (c == nullptr || b == nullptr || r == nullptr || valid_opts(o) != PCPPX_OK)
			return PCPPX_E_INVAL;
		r->layout = o->layout;  // set for an empty batch too: a reused records struct keeps no stale count
		r->layers_written = 0;
		if (b->n == 0)
			return PCPPX_OK;
		if (b->data == nullptr || b->offsets == nullptr || b->caplens == nullptr ||
		    (r->summary == nullptr && r->brief == nullptr) || (o->max_layers != 0 && r->layers == nullptr))
			return PCPPX_E_INVAL;
		// device-path-only outputs
		if (r->tuples != nullptr || r->proto_stats != nullptr || o->layout == PCPPX_LAYOUT_PACKED)
			return PCPPX_E_INVAL;
		// DENSE positions are 32-bit (the device's running totals, the facade's per-page indexes): a batch whose
		// n * max_layers could exceed them is refused rather than wrapped
		if (o->layout == PCPPX_LAYOUT_DENSE && (uint64_t)b->n * o->max_layers > (uint64_t)UINT32_MAX)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		int rc = init_host_path(c);
		if (rc != PCPPX_OK)
			return rc;
		abandon_slots(c);
		rc = parse_host_run(c, b, o, r);
		if (rc != PCPPX_OK)
			abandon_slots(c);
		return rc;
	}

	int pcppx_filter_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                        const pcppx_match_spec* spec, uint64_t seq_base, uint64_t* flow_keys, uint64_t* flow_first,
	                        uint32_t capacity, uint8_t* matched, pcppx_packet_stats* stats, void* hip_stream)
	{
		if (c == nullptr || b == nullptr || r == nullptr || spec == nullptr || max_layers == 0 ||
		    max_layers > PCPPX_MAX_LAYERS || capacity == 0 || (capacity & (capacity - 1)) != 0)
			return PCPPX_E_INVAL;
		if (b->n == 0)
			return PCPPX_OK;
		if (b->data == nullptr || b->offsets == nullptr || r->summary == nullptr || r->layers == nullptr ||
		    flow_keys == nullptr || flow_first == nullptr || matched == nullptr || stats == nullptr ||
		    r->layout != PCPPX_LAYOUT_FIXED)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		return pcppx::launch_filter(b, r, max_layers, spec, seq_base, flow_keys, flow_first, capacity, matched, stats,
		                            static_cast<hipStream_t>(hip_stream));
	}

	int pcppx_parse_batch_device_reasm(pcppx_ctx* c, const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r,
	                                   pcppx_reasm_info* info, void* hip_stream)
	{
		if (c == nullptr || b == nullptr || r == nullptr || valid_opts(o) != PCPPX_OK || o->max_layers == 0 ||
		    o->layout != PCPPX_LAYOUT_FIXED)
			return PCPPX_E_INVAL;
		if (b->n == 0)
			return PCPPX_OK;
		if (b->data == nullptr || b->offsets == nullptr || b->caplens == nullptr || r->summary == nullptr ||
		    r->layers == nullptr || info == nullptr)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		r->layout = PCPPX_LAYOUT_FIXED;
		return device_parse(c, b, o, r, info, static_cast<hipStream_t>(hip_stream));
	}

	int pcppx_reasm_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                       pcppx_reasm_info* info, void* hip_stream)
	{
		if (c == nullptr || b == nullptr || r == nullptr || max_layers == 0 || max_layers > PCPPX_MAX_LAYERS)
			return PCPPX_E_INVAL;
		if (b->n == 0)
			return PCPPX_OK;
		if (b->data == nullptr || b->offsets == nullptr || r->summary == nullptr || r->layers == nullptr ||
		    info == nullptr || r->layout != PCPPX_LAYOUT_FIXED)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		return pcppx::launch_reasm(b, r, max_layers, info, static_cast<hipStream_t>(hip_stream));
	}

	int pcppx_filter_reset(pcppx_ctx* c, uint32_t capacity)
	{
		if (c == nullptr || (capacity & (capacity - 1)) != 0)
			return PCPPX_E_INVAL;
		if (capacity == 0)
			capacity = kDefaultFlowSlots;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		for (Slot& s : c->slots)
			if (s.st && !ok(hipStreamSynchronize(s.st)))
				return PCPPX_E_HIP;
		if (capacity != c->flow_slots)
		{
			free_filter(c);
			if (!ok(hipMalloc(reinterpret_cast<void**>(&c->d_keys), (size_t)capacity * 8)) ||
			    !ok(hipMalloc(reinterpret_cast<void**>(&c->d_first), (size_t)capacity * 8)) ||
			    !ok(hipMalloc(reinterpret_cast<void**>(&c->d_stats), sizeof(pcppx_packet_stats))))
			{
				free_filter(c);
				return PCPPX_E_NOMEM;
			}
			c->flow_slots = capacity;
		}
		c->seq = 0;
		const bool good = ok(hipMemsetAsync(c->d_keys, 0, (size_t)capacity * 8, c->stream)) &&
		                  ok(hipMemsetAsync(c->d_first, 0, (size_t)capacity * 8, c->stream)) &&
		                  ok(hipMemsetAsync(c->d_stats, 0, sizeof(pcppx_packet_stats), c->stream)) &&
		                  ok(hipStreamSynchronize(c->stream));
		return good ? PCPPX_OK : PCPPX_E_HIP;
	}

	int pcppx_filter_batch_host(pcppx_ctx* c, const pcppx_batch* b, const pcppx_match_spec* spec, uint8_t* matched,
	                            pcppx_packet_stats* stats)
	{
		if (c == nullptr || b == nullptr || spec == nullptr)
			return PCPPX_E_INVAL;
		if (b->n != 0 && (b->data == nullptr || b->offsets == nullptr || b->caplens == nullptr || matched == nullptr))
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		int rc = c->flow_slots ? PCPPX_OK : pcppx_filter_reset(c, 0);
		if (rc == PCPPX_OK)
			rc = init_host_path(c);
		if (rc != PCPPX_OK)
			return rc;
		abandon_slots(c);
		rc = filter_host_run(c, b, spec, matched, stats);
		if (rc != PCPPX_OK)
			abandon_slots(c);
		return rc;
	}

	int pcppx_flow_count_device(pcppx_ctx* c, const pcppx_summary* summary, const uint32_t* caplens, uint32_t n,
	                            uint32_t* keys, uint64_t* packets, uint64_t* bytes, uint32_t capacity,
	                            uint64_t* stats, void* hip_stream)
	{
		return flow_count(c, summary, nullptr, caplens, n, keys, packets, bytes, capacity, stats, hip_stream);
	}

	int pcppx_flow_count_keys_device(pcppx_ctx* c, const uint32_t* keys_in, const uint32_t* caplens, uint32_t n,
	                                 uint32_t* keys, uint64_t* packets, uint64_t* bytes, uint32_t capacity,
	                                 uint64_t* stats, void* hip_stream)
	{
		return flow_count(c, nullptr, keys_in, caplens, n, keys, packets, bytes, capacity, stats, hip_stream);
	}
}

namespace
{
// pcppx_flow_count_device / _keys_device: keys from the summaries or from a dense column (exactly one non-null)
int flow_count(pcppx_ctx* c, const pcppx_summary* summary, const uint32_t* keys_in, const uint32_t* caplens, uint32_t n,
               uint32_t* keys, uint64_t* packets, uint64_t* bytes, uint32_t capacity, uint64_t* stats, void* hip_stream)
{
		if (c == nullptr || capacity == 0 || (capacity & (capacity - 1)) != 0)
			return PCPPX_E_INVAL;
		if (n == 0)
			return PCPPX_OK;
		if ((summary == nullptr) == (keys_in == nullptr) || caplens == nullptr || keys == nullptr || packets == nullptr ||
		    bytes == nullptr || stats == nullptr)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		hipStream_t st = static_cast<hipStream_t>(hip_stream);
		const uint32_t parts = pcppx::flow_partitions(capacity);
		const uint32_t rec_cap = pcppx::flow_queue_capacity(n, capacity);
		// the context's previous flow work (possibly queued on another stream) owns the queues until it is done
		const int src = c->flow.acquire(st, (uint64_t)parts * rec_cap * 16);
		if (src != PCPPX_OK)
			return src;
		if (c->d_flow_fill == nullptr)
		{
			if (!ok(hipMallocAsync(reinterpret_cast<void**>(&c->d_flow_fill), 1024 * sizeof(uint32_t), st)) ||
			    !ok(hipMemsetAsync(c->d_flow_fill, 0, 1024 * sizeof(uint32_t), st)))
				return PCPPX_E_NOMEM;
		}
		const int rc = pcppx::launch_flow_count_part(summary, keys_in, caplens, n, keys, packets, bytes, capacity, stats,
		                                             c->flow.ptr, rec_cap, c->d_flow_fill, st);
		return rc != PCPPX_OK ? rc : c->flow.mark_used(st);
	}
}

namespace
{
// PCPPX_LAYOUT_PACKED -> FIXED, the chain lengths at n_layers[i * stride]
int unpack_packed(const uint8_t* n_layers, size_t stride, const pcppx_layer* packed, uint64_t n, uint32_t max_layers,
                  pcppx_layer* fixed)
{
	if (packed == nullptr || fixed == nullptr || max_layers == 0 || max_layers > PCPPX_PACKED_MAX_LAYERS)
		return PCPPX_E_INVAL;
	uint64_t pos = 0;
	for (uint64_t i = 0; i < n; ++i)
	{
		if (i % 64 == 0)
			pos = i * max_layers;  // tile t's run starts at entry 64 * t * max_layers
		const uint32_t nl = n_layers[i * stride];
		const uint32_t cnt = nl < max_layers ? nl : max_layers;
		for (uint32_t k = 0; k < max_layers; ++k)
			fixed[i * max_layers + k] = k < cnt ? packed[pos + k] : pcppx_layer{};
		pos += cnt;
	}
	return PCPPX_OK;
}
}  // namespace

extern "C"
{
	void* pcppx_host_alloc(size_t bytes)
	{
		void* p = nullptr;
		if (hipHostMalloc(&p, bytes ? bytes : 1) != hipSuccess)
			return nullptr;
		return p;
	}

	void pcppx_host_free(void* p)
	{
		if (p)
			(void)hipHostFree(p);
	}

	int pcppx_unpack_layers(const pcppx_summary* summary, const pcppx_layer* packed, uint64_t n, uint32_t max_layers,
	                        pcppx_layer* fixed)
	{
		if (n == 0)
			return PCPPX_OK;
		if (summary == nullptr)
			return PCPPX_E_INVAL;
		return unpack_packed(&summary->n_layers, sizeof(pcppx_summary), packed, n, max_layers, fixed);
	}

	int pcppx_unpack_layers_brief(const pcppx_brief* brief, const pcppx_layer* packed, uint64_t n, uint32_t max_layers,
	                              pcppx_layer* fixed)
	{
		if (n == 0)
			return PCPPX_OK;
		if (brief == nullptr)
			return PCPPX_E_INVAL;
		return unpack_packed(&brief->n_layers, sizeof(pcppx_brief), packed, n, max_layers, fixed);
	}
}

namespace
{
// a device-batch operator's batch (non-null): empty, or with descriptors and, unless data_len is 0, bytes
bool valid_batch(const pcppx_batch* b)
{
	return b->n == 0 || (b->offsets != nullptr && b->caplens != nullptr && (b->data != nullptr || b->data_len == 0));
}

// The descriptor rule, as the host references apply it (the kernels': move::out_of_bounds in pcppx_move.h): packet i is
// out of bounds (true) when offsets[i] + caplens[i] wraps or exceeds data_len; else off = its source offset and
// len = min(caplen, snaplen), snaplen 0 = no limit.
bool out_of_bounds(const pcppx_batch* b, uint32_t snaplen, uint32_t i, uint64_t& off, uint32_t& len)
{
	off = b->offsets[i];
	const uint32_t cap = b->caplens[i];
	if (off + cap < off || off + cap > b->data_len)
		return true;
	len = (snaplen != 0 && cap > snaplen) ? snaplen : cap;
	return false;
}

// the argument rules pcppx_select_device and pcppx_select_reference share (include/pcppx.h)
bool valid_select(const pcppx_batch* b, const pcppx_select_spec* s, const pcppx_selection* o)
{
	if (b == nullptr || s == nullptr || o == nullptr || o->totals == nullptr || o->offsets == nullptr ||
	    o->caplens == nullptr)
		return false;
	if ((s->keep == nullptr) == (s->flags == nullptr))
		return false;
	if (s->flags != nullptr && s->flags_stride != sizeof(pcppx_brief) && s->flags_stride != sizeof(pcppx_summary))
		return false;
	if (s->invert > 1 || s->reserved != 0 || s->reserved2 != 0 || o->reserved != 0)
		return false;
	return valid_batch(b);
}
}  // namespace

extern "C"
{
	int pcppx_select_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_select_spec* s, pcppx_selection* o,
	                        void* hip_stream)
	{
		if (c == nullptr || !valid_select(b, s, o))
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		hipStream_t st = static_cast<hipStream_t>(hip_stream);
		if (b->n == 0)
			return ok(hipMemsetAsync(o->totals, 0, PCPPX_SEL_TOTALS * sizeof(uint64_t), st)) ? PCPPX_OK : PCPPX_E_HIP;
		// the context's previous select (possibly queued on another stream) owns the block sums until it is done
		int rc = c->select.acquire(st, pcppx::select_scratch_bytes(b->n));
		if (rc != PCPPX_OK)
			return rc;
		rc = pcppx::launch_select(b, s, o, c->select.ptr, st);
		return rc != PCPPX_OK ? rc : c->select.mark_used(st);
	}

	int pcppx_select_reference(const pcppx_batch* b, const pcppx_select_spec* s, pcppx_selection* o)
	{
		if (!valid_select(b, s, o))
			return PCPPX_E_INVAL;
		uint64_t sel = 0, sel_bytes = 0, written = 0, written_bytes = 0, bad = 0;
		bool open = true;  // every selected packet so far was written
		for (uint32_t i = 0; i < b->n; ++i)
		{
			bool chosen;
			if (s->keep != nullptr)
				chosen = s->keep[i] != 0;
			else
			{
				uint16_t f;
				std::memcpy(&f, static_cast<const uint8_t*>(s->flags) + (size_t)i * s->flags_stride, sizeof(f));
				chosen = (f & s->flags_any) != 0;
			}
			if (chosen == (s->invert != 0))
				continue;
			uint64_t off;
			uint32_t len;
			if (out_of_bounds(b, s->snaplen, i, off, len))
			{
				++bad;
				continue;
			}
			open = open && sel < o->max_packets && (o->data == nullptr || sel_bytes + len <= o->data_cap);
			if (open)
			{
				o->offsets[sel] = sel_bytes;
				o->caplens[sel] = len;
				if (o->index != nullptr)
					o->index[sel] = i;
				if (o->data != nullptr && len != 0)
					std::memcpy(o->data + sel_bytes, b->data + off, len);
				++written;
				written_bytes += len;
			}
			++sel;
			sel_bytes += len;
		}
		for (int k = 0; k < PCPPX_SEL_TOTALS; ++k)
			o->totals[k] = 0;
		o->totals[PCPPX_SEL_SELECTED_PACKETS] = sel;
		o->totals[PCPPX_SEL_SELECTED_BYTES] = sel_bytes;
		o->totals[PCPPX_SEL_WRITTEN_PACKETS] = written;
		o->totals[PCPPX_SEL_WRITTEN_BYTES] = written_bytes;
		o->totals[PCPPX_SEL_BAD_DESC] = bad;
		return PCPPX_OK;
	}
}

namespace
{
// the argument rules pcppx_steer_device and pcppx_steer_reference share (include/pcppx.h)
bool valid_steer(const pcppx_batch* b, const pcppx_steer_spec* s, const pcppx_steering* o)
{
	if (b == nullptr || s == nullptr || o == nullptr || o->totals == nullptr || o->offsets == nullptr ||
	    o->caplens == nullptr || o->bucket_first == nullptr || o->bucket_pos == nullptr)
		return false;
	if ((s->bucket == nullptr) == (s->key == nullptr))
		return false;
	if (s->n_buckets == 0 || s->n_buckets > PCPPX_STEER_MAX_BUCKETS)
		return false;
	if (s->key != nullptr && (s->key_stride < 4 || s->key_stride > 256 || s->key_stride % 4 != 0 ||
	                          reinterpret_cast<uintptr_t>(s->key) % 4 != 0))
		return false;
	if (s->reserved != 0 || o->reserved != 0)
		return false;
	return valid_batch(b);
}
}  // namespace

extern "C"
{
	int pcppx_steer_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_steer_spec* s, pcppx_steering* o,
	                       void* hip_stream)
	{
		if (c == nullptr || !valid_steer(b, s, o))
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		hipStream_t st = static_cast<hipStream_t>(hip_stream);
		if (b->n == 0)
			return ok(hipMemsetAsync(o->totals, 0, PCPPX_STEER_TOTALS * sizeof(uint64_t), st)) &&
			               ok(hipMemsetAsync(o->bucket_first, 0, (s->n_buckets + 1) * sizeof(uint32_t), st)) &&
			               ok(hipMemsetAsync(o->bucket_pos, 0, (s->n_buckets + 1) * sizeof(uint64_t), st))
			           ? PCPPX_OK
			           : PCPPX_E_HIP;
		// the context's previous steer (possibly queued on another stream) owns the block sums until it is done
		int rc = c->steer.acquire(st, pcppx::steer_scratch_bytes(b->n, s->n_buckets));
		if (rc != PCPPX_OK)
			return rc;
		rc = pcppx::launch_steer(b, s, o, c->steer.ptr, st);
		return rc != PCPPX_OK ? rc : c->steer.mark_used(st);
	}

	int pcppx_steer_reference(const pcppx_batch* b, const pcppx_steer_spec* s, pcppx_steering* o)
	{
		if (!valid_steer(b, s, o))
			return PCPPX_E_INVAL;
		const uint32_t K = s->n_buckets;
		constexpr uint32_t kNone = 0xFFFFFFFFu;
		uint64_t dropped = 0, bad = 0;
		// pass 1: every packet's bucket (kNone: not steered) and output length; the buckets' packets and bytes
		std::vector<uint32_t> bucket(b->n), len(b->n), first(K + 1, 0);
		std::vector<uint64_t> pos(K + 1, 0);
		for (uint32_t i = 0; i < b->n; ++i)
		{
			uint32_t v;
			if (s->bucket != nullptr)
				v = s->bucket[i];
			else
			{
				std::memcpy(&v, static_cast<const uint8_t*>(s->key) + (size_t)i * s->key_stride, sizeof(v));
				v %= K;
			}
			bucket[i] = kNone;
			len[i] = 0;
			if (v >= K)
			{
				++dropped;
				continue;
			}
			uint64_t off;
			if (out_of_bounds(b, s->snaplen, i, off, len[i]))
			{
				++bad;
				continue;
			}
			bucket[i] = v;
			++first[v + 1];
			pos[v + 1] += len[i];
		}
		for (uint32_t k = 0; k < K; ++k)
		{
			first[k + 1] += first[k];
			pos[k + 1] += pos[k];
		}
		const bool overflow = first[K] > o->max_packets || (o->data != nullptr && pos[K] > o->data_cap);
		for (uint32_t k = 0; k <= K; ++k)
		{
			o->bucket_first[k] = first[k];
			o->bucket_pos[k] = pos[k];
		}
		for (int k = 0; k < PCPPX_STEER_TOTALS; ++k)
			o->totals[k] = 0;
		o->totals[PCPPX_STEER_STEERED_PACKETS] = first[K];
		o->totals[PCPPX_STEER_STEERED_BYTES] = pos[K];
		o->totals[PCPPX_STEER_DROPPED] = dropped;
		o->totals[PCPPX_STEER_BAD_DESC] = bad;
		o->totals[PCPPX_STEER_OVERFLOW] = overflow ? 1 : 0;
		if (overflow)  // all or nothing
			return PCPPX_OK;
		// pass 2: each packet behind the packets of its bucket before it (first / pos: the buckets' next places)
		for (uint32_t i = 0; i < b->n; ++i)
		{
			const uint32_t v = bucket[i];
			if (v == kNone)
				continue;
			const uint32_t r = first[v]++;
			const uint64_t p = pos[v];
			pos[v] += len[i];
			o->offsets[r] = p;
			o->caplens[r] = len[i];
			if (o->index != nullptr)
				o->index[r] = i;
			if (o->data != nullptr && len[i] != 0)
				std::memcpy(o->data + p, b->data + b->offsets[i], len[i]);
		}
		return PCPPX_OK;
	}
}

// ---- defrag: the IPv4 / IPv6 fragment groups that are complete inside a batch (include/pcppx.h, defrag, defrag6) ----
namespace
{
// a spec of either entry point: pcppx_defrag_spec is families = V4
struct DefragRules
{
	uint32_t max_fragments, passthrough, families;
};

// the argument rules the four defrag calls share but for the spec's own fields (include/pcppx.h)
bool valid_defrag_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_reasm_info* info,
                       const pcppx_defragged* o)
{
	if (b == nullptr || r == nullptr || o == nullptr || o->totals == nullptr || o->offsets == nullptr ||
	    o->caplens == nullptr)
		return false;
	if (max_layers == 0 || max_layers > PCPPX_MAX_LAYERS || r->layout != PCPPX_LAYOUT_FIXED)
		return false;
	if (o->reserved != 0)
		return false;
	if (b->n != 0 && (info == nullptr || r->layers == nullptr || (r->summary == nullptr && r->brief == nullptr)))
		return false;
	return valid_batch(b);
}

// the argument rules pcppx_defrag_device and pcppx_defrag_reference share
bool valid_defrag(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_reasm_info* info,
                  const pcppx_defrag_spec* s, const pcppx_defragged* o, DefragRules& rules)
{
	if (s == nullptr || s->passthrough > 1 || s->reserved[0] != 0 || s->reserved[1] != 0 || s->reserved[2] != 0)
		return false;
	rules = { s->max_fragments, s->passthrough, PCPPX_DEFRAG_FAM_V4 };
	return valid_defrag_args(b, r, max_layers, info, o);
}

// and the ones pcppx_defrag6_device and pcppx_defrag6_reference share
bool valid_defrag6(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_reasm_info* info,
                   const pcppx_defrag6_spec* s, const pcppx_defragged* o, DefragRules& rules)
{
	if (s == nullptr || s->passthrough > 1 || s->reserved[0] != 0 || s->reserved[1] != 0 || s->families == 0 ||
	    s->families > (PCPPX_DEFRAG_FAM_V4 | PCPPX_DEFRAG_FAM_V6))
		return false;
	rules = { s->max_fragments, s->passthrough, s->families };
	return valid_defrag_args(b, r, max_layers, info, o);
}

// where the chain lengths are read from: the summary's n_layers, else the brief's
const uint8_t* n_layers_column(const pcppx_records* r, uint32_t& stride)
{
	if (r->summary != nullptr)
	{
		stride = sizeof(pcppx_summary);
		return &r->summary->n_layers;
	}
	stride = sizeof(pcppx_brief);
	return &r->brief->n_layers;
}

// pcppx_defrag_device and pcppx_defrag6_device behind their argument checks
int defrag_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                  const pcppx_reasm_info* info, const DefragRules& s, pcppx_defragged* o, void* hip_stream)
{
	if (!ok(hipSetDevice(c->device)))
		return PCPPX_E_HIP;
	hipStream_t st = static_cast<hipStream_t>(hip_stream);
	if (b->n == 0)
		return ok(hipMemsetAsync(o->totals, 0, PCPPX_DEFRAG_TOTALS * sizeof(uint64_t), st)) ? PCPPX_OK : PCPPX_E_HIP;
	// the context's previous defrag (possibly queued on another stream) owns the table until it is done
	int rc = c->defrag.acquire(st, pcppx::defrag_scratch_bytes(b->n, s.max_fragments));
	if (rc != PCPPX_OK)
		return rc;
	uint32_t stride;
	const uint8_t* nl = n_layers_column(r, stride);
	rc = pcppx::launch_defrag(b, r->layers, max_layers, nl, stride, info, s.max_fragments, s.passthrough, s.families,
	                          o, c->defrag.ptr, st);
	return rc != PCPPX_OK ? rc : c->defrag.mark_used(st);
}

// the next-header values parseExtensions (IPv6Layer.cpp:79-147) takes for an extension
bool is_v6_extension(uint32_t nh)
{
	return nh == 0 || nh == 43 || nh == 44 || nh == 51 || nh == 60;
}

// parseExtensions over the extensions ip[40, hdr) of an IPv6 header (hdr >= 48, inside the packet): true iff the chain
// ends exactly at hdr, holds a fragment header and does not go on behind hdr. nh: the last extension's next header.
bool walk_v6_chain(const uint8_t* ip, uint32_t hdr, uint32_t& nh)
{
	nh = ip[6];
	uint32_t at = 40;
	bool frag = false;
	while (at + 2 <= hdr && is_v6_extension(nh))
	{
		const uint32_t len8 = ip[at + 1];
		frag = frag || nh == 44;
		const uint32_t ext = nh == 44 ? 8u : nh == 51 ? (len8 + 2) * 4 : (len8 + 1) * 8;
		nh = ip[at];
		at += ext;
	}
	return at == hdr && frag && !is_v6_extension(nh);
}

// pcppx_defrag_reference and pcppx_defrag6_reference behind their argument checks: one set of group rules
int defrag_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_reasm_info* info,
                     const DefragRules* s, pcppx_defragged* o)
{
	const uint32_t n = b->n;
	struct Frag
	{
		uint32_t idx, foff, len, ip_off, hdr;
		bool last, v6;
	};
	// every packet's disposition; the candidates by key, in source order
	std::vector<uint8_t> disp(n, PCPPX_DEFRAG_PASS);
	std::map<uint32_t, std::vector<Frag>> groups;
	uint64_t candidates = 0, bad = 0;
	uint32_t stride = 0;
	const uint8_t* nlc = n != 0 ? n_layers_column(r, stride) : nullptr;
	for (uint32_t i = 0; i < n; ++i)
	{
		uint64_t off;
		uint32_t cap;
		if (out_of_bounds(b, 0, i, off, cap))
		{
			disp[i] = PCPPX_DEFRAG_BAD_DESC;
			++bad;
			continue;
		}
		const uint8_t st = info[i].ip_status;
		if ((st & 15) != PCPPX_IPR_FRAGMENT)
			continue;
		disp[i] = PCPPX_DEFRAG_LEFT;  // until its group turns out clean
		// families = V4: an IPv6 fragment stays outside the groups. Else both families form them, and the one the spec
		// does not ask for keeps its groups (and those it shares a key with) from being clean
		const bool v6 = (st & PCPPX_IPR_F_IPV6) != 0;
		if (v6 && s->families == PCPPX_DEFRAG_FAM_V4)
			continue;
		const uint32_t proto = v6 ? 3 : 2, min_hdr = v6 ? 48 : 20;  // pcpp::IPv6 / pcpp::IPv4: the first such layer
		const uint32_t nl = std::min<uint32_t>(nlc[(size_t)i * stride], max_layers);
		for (uint32_t k = 0; k < nl; ++k)
		{
			const pcppx_layer& L = r->layers[(size_t)i * max_layers + k];
			if (L.proto != proto)
				continue;
			if (L.hdr_len >= min_hdr && L.hdr_len <= L.data_len && (uint32_t)L.offset + L.data_len <= cap)
			{
				groups[info[i].ip_key].push_back({ i, info[i].frag_offset, (uint32_t)(L.data_len - L.hdr_len), L.offset,
				                                   L.hdr_len, (st & PCPPX_IPR_F_LAST) != 0, v6 });
				++candidates;
			}
			break;
		}
	}
	for (int k = 0; k < PCPPX_DEFRAG_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_DEFRAG_CANDIDATES] = candidates;
	o->totals[PCPPX_DEFRAG_BAD_DESC_N] = bad;
	if (candidates > (s->max_fragments == 0 ? n : s->max_fragments))  // no room to form the groups
	{
		o->totals[PCPPX_DEFRAG_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	// the clean groups: members sorted by (frag_offset, source index), keyed by the completing member
	struct Packet
	{
		std::vector<Frag> members;
		uint32_t total;
	};
	std::map<uint32_t, Packet> done;
	uint64_t merged = 0;
	// what the packet keeps of the first member's IP header: an IPv6 one loses its extensions
	auto kept = [](const Frag& f) { return f.v6 ? 40u : f.hdr; };
	for (auto& kv : groups)
	{
		std::vector<Frag>& m = kv.second;
		if (m.size() < 2 || m.size() > PCPPX_DEFRAG_MAX_FRAGS)
			continue;
		std::sort(m.begin(), m.end(),
		          [](const Frag& x, const Frag& y) { return x.foff != y.foff ? x.foff < y.foff : x.idx < y.idx; });
		uint32_t total = 0;
		bool clean = true;
		for (size_t k = 0; k < m.size() && clean; ++k)
		{
			clean = m[k].len > 0 && m[k].foff == total && m[k].last == (k + 1 == m.size()) && m[k].v6 == m[0].v6;
			total += m[k].len;
		}
		if (!clean || m[0].ip_off + m[0].hdr + total > PCPPX_MAX_CAPLEN || m[0].hdr + total > 65535)
			continue;
		if ((s->families & (m[0].v6 ? PCPPX_DEFRAG_FAM_V6 : PCPPX_DEFRAG_FAM_V4)) == 0)
			continue;
		uint32_t nh;
		if (m[0].v6 && !walk_v6_chain(b->data + b->offsets[m[0].idx] + m[0].ip_off, m[0].hdr, nh))
			continue;
		uint32_t at = 0;
		for (const Frag& f : m)
		{
			disp[f.idx] = PCPPX_DEFRAG_MERGED;
			at = std::max(at, f.idx);
		}
		disp[at] = PCPPX_DEFRAG_MERGED_LAST;
		merged += m.size();
		done[at] = Packet{ m, total };
	}
	// the output's size, then (all or nothing) the output itself, in source order
	uint64_t out_packets = 0, out_bytes = 0, left = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		left += disp[i] == PCPPX_DEFRAG_LEFT;
		if (disp[i] == PCPPX_DEFRAG_MERGED_LAST)
		{
			const Packet& p = done[i];
			++out_packets;
			out_bytes += p.members[0].ip_off + kept(p.members[0]) + p.total;
		}
		else if (s->passthrough && (disp[i] == PCPPX_DEFRAG_PASS || disp[i] == PCPPX_DEFRAG_LEFT))
		{
			++out_packets;
			out_bytes += b->caplens[i];
		}
	}
	const bool overflow = out_packets > o->max_packets || (o->data != nullptr && out_bytes > o->data_cap);
	o->totals[PCPPX_DEFRAG_OUT_PACKETS] = out_packets;
	o->totals[PCPPX_DEFRAG_OUT_BYTES] = out_bytes;
	o->totals[PCPPX_DEFRAG_REASSEMBLED] = done.size();
	o->totals[PCPPX_DEFRAG_MERGED_FRAGS] = merged;
	o->totals[PCPPX_DEFRAG_LEFT_FRAGS] = left;
	o->totals[PCPPX_DEFRAG_OVERFLOW] = overflow ? 1 : 0;
	if (overflow)
		return PCPPX_OK;
	uint32_t j = 0;
	uint64_t pos = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		if (o->disposition != nullptr)
			o->disposition[i] = disp[i];
		uint32_t len, first = i;
		uint8_t frags = 0;
		if (disp[i] == PCPPX_DEFRAG_MERGED_LAST)
		{
			const Packet& p = done[i];
			const Frag& f = p.members[0];
			len = f.ip_off + kept(f) + p.total;
			first = f.idx;
			frags = (uint8_t)p.members.size();
			if (o->data != nullptr)
			{
				uint8_t* d = o->data + pos;
				std::memcpy(d, b->data + b->offsets[f.idx], f.ip_off + kept(f));
				for (const Frag& x : p.members)
					std::memcpy(d + f.ip_off + kept(f) + x.foff, b->data + b->offsets[x.idx] + x.ip_off + x.hdr, x.len);
				uint8_t* ip = d + f.ip_off;
				const uint32_t tot_len = f.hdr + p.total;
				if (f.v6)
				{
					// IPReassembly.cpp:476 stores hdr + total without htobe16, the parse of :481 clamps the layer to
					// that value read as big-endian (IPv6Layer.cpp:37-39), computeCalculateFields writes it back;
					// removeAllExtensions leaves the last extension's next header
					const uint32_t swapped = ((tot_len & 0xFFu) << 8) | (tot_len >> 8);
					const uint32_t plen = std::min(p.total, swapped);
					uint32_t nh;
					walk_v6_chain(b->data + b->offsets[f.idx] + f.ip_off, f.hdr, nh);
					ip[4] = (uint8_t)(plen >> 8);
					ip[5] = (uint8_t)plen;
					ip[6] = (uint8_t)nh;
				}
				else
				{
					// the header as computeCalculateFields leaves it: total length, no fragment word, the checksum
					ip[2] = (uint8_t)(tot_len >> 8);
					ip[3] = (uint8_t)tot_len;
					ip[6] = ip[7] = ip[10] = ip[11] = 0;
					uint32_t sum = 0;
					for (uint32_t k = 0; k < f.hdr; k += 2)
						sum += ((uint32_t)ip[k] << 8) | (k + 1 < f.hdr ? ip[k + 1] : 0u);
					while (sum >> 16)
						sum = (sum & 0xFFFFu) + (sum >> 16);
					ip[10] = (uint8_t)(~sum >> 8);
					ip[11] = (uint8_t)~sum;
				}
			}
		}
		else if (s->passthrough && (disp[i] == PCPPX_DEFRAG_PASS || disp[i] == PCPPX_DEFRAG_LEFT))
		{
			len = b->caplens[i];
			if (o->data != nullptr && len != 0)
				std::memcpy(o->data + pos, b->data + b->offsets[i], len);
		}
		else
			continue;
		o->offsets[j] = pos;
		o->caplens[j] = len;
		if (o->index != nullptr)
			o->index[j] = i;
		if (o->first != nullptr)
			o->first[j] = first;
		if (o->frags != nullptr)
			o->frags[j] = frags;
		++j;
		pos += len;
	}
	return PCPPX_OK;
}
}  // namespace

extern "C"
{
	int pcppx_defrag_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                        const pcppx_reasm_info* info, const pcppx_defrag_spec* s, pcppx_defragged* o,
	                        void* hip_stream)
	{
		DefragRules rules;
		if (c == nullptr || !valid_defrag(b, r, max_layers, info, s, o, rules))
			return PCPPX_E_INVAL;
		return defrag_device(c, b, r, max_layers, info, rules, o, hip_stream);
	}

	int pcppx_defrag_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                           const pcppx_reasm_info* info, const pcppx_defrag_spec* s, pcppx_defragged* o)
	{
		DefragRules rules;
		if (!valid_defrag(b, r, max_layers, info, s, o, rules))
			return PCPPX_E_INVAL;
		return defrag_reference(b, r, max_layers, info, &rules, o);
	}

	int pcppx_defrag6_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                         const pcppx_reasm_info* info, const pcppx_defrag6_spec* s, pcppx_defragged* o,
	                         void* hip_stream)
	{
		DefragRules rules;
		if (c == nullptr || !valid_defrag6(b, r, max_layers, info, s, o, rules))
			return PCPPX_E_INVAL;
		return defrag_device(c, b, r, max_layers, info, rules, o, hip_stream);
	}

	int pcppx_defrag6_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                            const pcppx_reasm_info* info, const pcppx_defrag6_spec* s, pcppx_defragged* o)
	{
		DefragRules rules;
		if (!valid_defrag6(b, r, max_layers, info, s, o, rules))
			return PCPPX_E_INVAL;
		return defrag_reference(b, r, max_layers, info, &rules, o);
	}
}

// ---- tcpstream: the TCP connection sides that are clean inside a batch (include/pcppx.h, tcpstream) ----
namespace pcppx
{
// pcppx_tcpstream_ref.cpp (plain C++, beside pcppx_tcpstream_reference): the argument rules both calls share
bool valid_tcpstream(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_reasm_info* info,
                     const pcppx_tcpstream_spec* s, const pcppx_tcpstreams* o);
}  // namespace pcppx

extern "C"
{
	int pcppx_tcpstream_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                           const pcppx_reasm_info* info, const pcppx_tcpstream_spec* s, pcppx_tcpstreams* o,
	                           void* hip_stream)
	{
		if (c == nullptr || !pcppx::valid_tcpstream(b, r, max_layers, info, s, o))
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		hipStream_t st = static_cast<hipStream_t>(hip_stream);
		if (b->n == 0)
			return ok(hipMemsetAsync(o->totals, 0, PCPPX_TCPS_TOTALS * sizeof(uint64_t), st)) ? PCPPX_OK : PCPPX_E_HIP;
		// the context's previous tcpstream call (possibly queued on another stream) owns the tables until it is done
		int rc = c->tcpstream.acquire(st, pcppx::tcpstream_scratch_bytes(b->n, s->max_segments));
		if (rc != PCPPX_OK)
			return rc;
		const uint8_t* rec0 = r->summary != nullptr ? reinterpret_cast<const uint8_t*>(r->summary)
		                                            : reinterpret_cast<const uint8_t*>(r->brief);
		const uint32_t stride = r->summary != nullptr ? sizeof(pcppx_summary) : sizeof(pcppx_brief);
		rc = pcppx::launch_tcpstream(b, r->layers, max_layers, rec0, stride, info, s, o, c->tcpstream.ptr, st);
		return rc != PCPPX_OK ? rc : c->tcpstream.mark_used(st);
	}
}

// ---- the message operators: tlsfp, dns, http, ssl, sip, dhcp (include/pcppx.h) ----
// pcppx_<op>_reference is pcppx_<op>_ref.cpp (plain C++); the argument rules both calls share are pcppx_<op>.h's
namespace
{
// What the six device entries do once the arguments have their verdict (valid: with c there). scratch: the context's
// own for the operator, which its previous call (possibly queued on another stream) owns until it is done.
template <class Spec, class Out>
int message_device(pcppx_ctx* c, bool valid, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                   const Spec* s, const Out* o, uint32_t n_totals, Scratch pcppx_ctx::*scratch,
                   uint64_t (*scratch_bytes)(uint32_t),
                   int (*launch)(const pcppx_batch*, const pcppx_layer*, uint32_t, const uint8_t*, uint32_t, const Spec*,
                                 const Out*, void*, hipStream_t),
                   void* hip_stream)
{
	if (!valid)
		return PCPPX_E_INVAL;
	if (!ok(hipSetDevice(c->device)))
		return PCPPX_E_HIP;
	hipStream_t st = static_cast<hipStream_t>(hip_stream);
	if (b->n == 0)
		return ok(hipMemsetAsync(o->totals, 0, n_totals * sizeof(uint64_t), st)) ? PCPPX_OK : PCPPX_E_HIP;
	Scratch& sc = c->*scratch;
	int rc = sc.acquire(st, scratch_bytes(b->n));
	if (rc != PCPPX_OK)
		return rc;
	const uint8_t* rec0 = r->summary != nullptr ? reinterpret_cast<const uint8_t*>(r->summary)
	                                            : reinterpret_cast<const uint8_t*>(r->brief);
	const uint32_t stride = r->summary != nullptr ? sizeof(pcppx_summary) : sizeof(pcppx_brief);
	rc = launch(b, r->layers, max_layers, rec0, stride, s, o, sc.ptr, st);
	return rc != PCPPX_OK ? rc : sc.mark_used(st);
}
}  // namespace

extern "C"
{
	int pcppx_tlsfp_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                       const pcppx_tlsfp_spec* s, pcppx_tlsfps* o, void* hip_stream)
	{
		return message_device<pcppx_tlsfp_spec, pcppx_tlsfps>(
		    c, c != nullptr && pcppx::tlsfp::valid_args(b, r, max_layers, s, o), b, r, max_layers, s, o,
		    PCPPX_TLSFP_TOTALS, &pcppx_ctx::tlsfp, pcppx::tlsfp_scratch_bytes, pcppx::launch_tlsfp, hip_stream);
	}

	int pcppx_dns_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                     const pcppx_dns_spec* s, pcppx_dns_out* o, void* hip_stream)
	{
		return message_device<pcppx_dns_spec, pcppx_dns_out>(
		    c, c != nullptr && pcppx::dns::valid_args(b, r, max_layers, s, o), b, r, max_layers, s, o, PCPPX_DNS_TOTALS,
		    &pcppx_ctx::dns, pcppx::dns_scratch_bytes, pcppx::launch_dns, hip_stream);
	}

	int pcppx_http_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                      const pcppx_http_spec* s, pcppx_http_out* o, void* hip_stream)
	{
		return message_device<pcppx_http_spec, pcppx_http_out>(
		    c, c != nullptr && pcppx::http::valid_args(b, r, max_layers, s, o), b, r, max_layers, s, o, PCPPX_HTTP_TOTALS,
		    &pcppx_ctx::http, pcppx::http_scratch_bytes, pcppx::launch_http, hip_stream);
	}

	int pcppx_ssl_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                     const pcppx_ssl_spec* s, pcppx_ssl_out* o, void* hip_stream)
	{
		return message_device<pcppx_ssl_spec, pcppx_ssl_out>(
		    c, c != nullptr && pcppx::ssl::valid_args(b, r, max_layers, s, o), b, r, max_layers, s, o, PCPPX_SSL_TOTALS,
		    &pcppx_ctx::ssl, pcppx::ssl_scratch_bytes, pcppx::launch_ssl, hip_stream);
	}

	int pcppx_sip_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                     const pcppx_sip_spec* s, pcppx_sip_out* o, void* hip_stream)
	{
		return message_device<pcppx_sip_spec, pcppx_sip_out>(
		    c, c != nullptr && pcppx::sip::valid_args(b, r, max_layers, s, o), b, r, max_layers, s, o, PCPPX_SIP_TOTALS,
		    &pcppx_ctx::sip, pcppx::sip_scratch_bytes, pcppx::launch_sip, hip_stream);
	}

	int pcppx_dhcp_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                      const pcppx_dhcp_spec* s, pcppx_dhcp_out* o, void* hip_stream)
	{
		return message_device<pcppx_dhcp_spec, pcppx_dhcp_out>(
		    c, c != nullptr && pcppx::dhcp::valid_args(b, r, max_layers, s, o), b, r, max_layers, s, o, PCPPX_DHCP_TOTALS,
		    &pcppx_ctx::dhcp, pcppx::dhcp_scratch_bytes, pcppx::launch_dhcp, hip_stream);
	}
}

// ---- frag: the IPv4 / IPv6 packets of a batch split into fragments (include/pcppx.h, frag, frag6) ----
namespace
{
// the argument rules the four frag calls share; a pcppx_frag_spec arrives as a pcppx_frag6_spec with families = V4
bool valid_frag6(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_frag6_spec* s,
                 const pcppx_fragmented* o)
{
	if (b == nullptr || r == nullptr || s == nullptr || o == nullptr || o->totals == nullptr || o->offsets == nullptr ||
	    o->caplens == nullptr)
		return false;
	if (max_layers == 0 || max_layers > PCPPX_MAX_LAYERS || r->layout != PCPPX_LAYOUT_FIXED)
		return false;
	if ((s->frag_size == 0) == (s->mtu == 0))
		return false;
	if (s->frag_size != 0 && (s->frag_size % 8 != 0 || s->frag_size > 65528))
		return false;
	if (s->mtu != 0 && (s->mtu < 68 || s->mtu > 65535))
		return false;
	if (s->copy_rest > 1 || s->honor_df > 1 || o->reserved != 0 || s->reserved2 != 0)
		return false;
	if (s->families == 0 || (s->families & ~(PCPPX_FRAG_FAM_V4 | PCPPX_FRAG_FAM_V6)) != 0)
		return false;
	for (uint8_t x : s->reserved)
		if (x != 0)
			return false;
	if (b->n != 0 && (r->layers == nullptr || (r->summary == nullptr && r->brief == nullptr)))
		return false;
	return valid_batch(b);
}

// pcppx_frag_spec as the spec both families share: families = V4, no ids. False where its own reserved bytes are set.
bool widen_frag_spec(const pcppx_frag_spec* s, pcppx_frag6_spec& w)
{
	w = pcppx_frag6_spec{};
	if (s == nullptr)
		return false;
	for (uint8_t x : s->reserved)
		if (x != 0)
			return false;
	w.keep = s->keep;
	w.frag_size = s->frag_size;
	w.mtu = s->mtu;
	w.copy_rest = s->copy_rest;
	w.honor_df = s->honor_df;
	w.families = PCPPX_FRAG_FAM_V4;
	return true;
}

// pcppx_frag_device and pcppx_frag6_device behind their argument checks
int frag_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                const pcppx_frag6_spec* s, pcppx_fragmented* o, void* hip_stream)
{
	if (!ok(hipSetDevice(c->device)))
		return PCPPX_E_HIP;
	hipStream_t st = static_cast<hipStream_t>(hip_stream);
	if (b->n == 0)
		return ok(hipMemsetAsync(o->totals, 0, PCPPX_FRAG_TOTALS * sizeof(uint64_t), st)) ? PCPPX_OK : PCPPX_E_HIP;
	// the context's previous frag (possibly queued on another stream) owns the plans until it is done
	int rc = c->frag.acquire(st, pcppx::frag_scratch_bytes(b->n));
	if (rc != PCPPX_OK)
		return rc;
	uint32_t stride;
	const uint8_t* nl = n_layers_column(r, stride);
	rc = pcppx::launch_frag(b, r->layers, max_layers, nl, stride, s, o, c->frag.ptr, st);
	return rc != PCPPX_OK ? rc : c->frag.mark_used(st);
}

// a source packet as both references see it
struct FragSrc
{
	uint8_t disp;
	bool v6;
	uint32_t ip_off, hdr, pay, fs, count;  // of a SPLIT packet
	uint32_t nh_at;                        // IPv6: the packet offset of the last next-header byte
};

// The disposition of in-bounds packet i (packet bytes pk, caplen cap) and, for a SPLIT packet, its shape: the one
// per-packet routine of pcppx_frag_reference and pcppx_frag6_reference.
uint8_t frag_classify(const pcppx_records* r, uint8_t max_layers, const uint8_t* nlc, uint32_t stride,
                      const pcppx_frag6_spec* s, uint32_t i, const uint8_t* pk, uint32_t cap, FragSrc& x)
{
	if (s->keep != nullptr && s->keep[i] == 0)
		return PCPPX_FRAG_UNSELECTED;
	const uint32_t nl = std::min<uint32_t>(nlc[(size_t)i * stride], max_layers);
	const pcppx_layer* L = nullptr;
	const pcppx_layer* L6 = nullptr;
	bool plain = true;  // every layer ahead of the IPv6 one is Ethernet, VLAN or SLL
	for (uint32_t k = 0; k < nl; ++k)
	{
		const pcppx_layer* X = &r->layers[(size_t)i * max_layers + k];
		if (X->proto == 2 && L == nullptr)  // pcpp::IPv4: the first such layer
			L = X;
		if (X->proto == 3 && L6 == nullptr)  // pcpp::IPv6
			L6 = X;
		if (L6 == nullptr)
			plain = plain && (X->proto == 1 || X->proto == 9 || X->proto == 19);
	}
	if (L != nullptr || (s->families & PCPPX_FRAG_FAM_V6) == 0)
	{
		if (L == nullptr || (s->families & PCPPX_FRAG_FAM_V4) == 0 || L->hdr_len < 20 || L->hdr_len > 60 ||
		    L->hdr_len > L->data_len || (uint32_t)L->offset + L->data_len > cap)
			return PCPPX_FRAG_NOT_V4;
		x.ip_off = L->offset;
		x.hdr = L->hdr_len;
		x.pay = (uint32_t)L->data_len - L->hdr_len;
		x.fs = s->frag_size != 0 ? s->frag_size : ((s->mtu - x.hdr) & ~7u);
		const uint8_t* ip = pk + x.ip_off;
		const uint32_t word = ((uint32_t)ip[6] << 8) | ip[7];
		if ((word & 0x3FFFu) != 0)
			return PCPPX_FRAG_ALREADY;
		if (s->frag_size != 0 ? x.pay <= x.fs : x.hdr + x.pay <= s->mtu)
			return PCPPX_FRAG_FITS;
		if (s->honor_df != 0 && (word & 0x4000u) != 0)
			return PCPPX_FRAG_DF;
		return PCPPX_FRAG_SPLIT;
	}
	if (L6 == nullptr || L6->hdr_len < 40 || L6->hdr_len > L6->data_len || (uint32_t)L6->offset + L6->data_len > cap)
		return PCPPX_FRAG_NOT_IP;
	x.v6 = true;
	x.ip_off = L6->offset;
	x.hdr = L6->hdr_len;
	x.pay = (uint32_t)L6->data_len - L6->hdr_len;
	// parseExtensions over [40, hdr): it must end exactly at hdr
	const uint8_t* ip = pk + x.ip_off;
	uint32_t nh = ip[6], at = 40, steps = 0;
	bool fragmented = false;
	x.nh_at = x.ip_off + 6;
	while (at < x.hdr)
	{
		if (!is_v6_extension(nh) || at + 2 > x.hdr)
			return PCPPX_FRAG_NOT_IP;
		if (steps++ == PCPPX_FRAG6_MAX_EXT)
			return PCPPX_FRAG_LEFT;
		const uint32_t len8 = ip[at + 1];
		fragmented = fragmented || nh == 44;
		x.nh_at = x.ip_off + at;
		const uint32_t ext = nh == 44 ? 8u : nh == 51 ? (len8 + 2) * 4 : (len8 + 1) * 8;
		nh = ip[at];
		at += ext;
	}
	if (at != x.hdr)
		return PCPPX_FRAG_NOT_IP;
	if (!plain)
		return PCPPX_FRAG_LEFT;
	if (fragmented)
		return PCPPX_FRAG_ALREADY;
	if (s->frag_size != 0 ? x.pay <= s->frag_size : x.hdr + x.pay <= s->mtu)
		return PCPPX_FRAG_FITS;
	if (s->frag_size == 0 && s->mtu < x.hdr + 16)
		return PCPPX_FRAG_LEFT;
	x.fs = s->frag_size != 0 ? s->frag_size : ((s->mtu - x.hdr - 8) & ~7u);
	return PCPPX_FRAG_SPLIT;
}

// pcppx_frag_reference and pcppx_frag6_reference behind their argument checks
int frag_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_frag6_spec* s,
                   pcppx_fragmented* o)
{
	const uint32_t n = b->n;
	std::vector<FragSrc> src(n);
	uint32_t stride = 0;
	const uint8_t* nlc = n != 0 ? n_layers_column(r, stride) : nullptr;
	uint64_t out_packets = 0, out_bytes = 0, split = 0, fragments = 0, copied = 0, fits = 0, bad = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		FragSrc& x = src[i];
		x = FragSrc{ PCPPX_FRAG_BAD_DESC, false, 0, 0, 0, 0, 0, 0 };
		uint64_t off;
		uint32_t cap;
		if (out_of_bounds(b, 0, i, off, cap))
		{
			++bad;
			continue;
		}
		x.disp = frag_classify(r, max_layers, nlc, stride, s, i, b->data + off, cap, x);
		fits += x.disp == PCPPX_FRAG_FITS;
		if (x.disp == PCPPX_FRAG_SPLIT)
		{
			x.count = (x.pay + x.fs - 1) / x.fs;
			++split;
			fragments += x.count;
			out_bytes += (uint64_t)x.count * (x.ip_off + x.hdr + (x.v6 ? 8u : 0u)) + x.pay;
		}
		else if (s->copy_rest != 0)
		{
			x.count = 1;
			++copied;
			out_bytes += cap;
		}
		out_packets += x.count;
	}
	const bool overflow = out_packets > o->max_packets || (o->data != nullptr && out_bytes > o->data_cap);
	o->totals[PCPPX_FRAG_OUT_PACKETS] = out_packets;
	o->totals[PCPPX_FRAG_OUT_BYTES] = out_bytes;
	o->totals[PCPPX_FRAG_SPLIT_PACKETS] = split;
	o->totals[PCPPX_FRAG_FRAGMENTS] = fragments;
	o->totals[PCPPX_FRAG_COPIED] = copied;
	o->totals[PCPPX_FRAG_UNDER_SIZE] = fits;
	o->totals[PCPPX_FRAG_BAD_DESC_N] = bad;
	o->totals[PCPPX_FRAG_OVERFLOW] = overflow ? 1 : 0;
	if (overflow)
		return PCPPX_OK;
	uint32_t j = 0;
	uint64_t pos = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		const FragSrc& x = src[i];
		if (o->disposition != nullptr)
			o->disposition[i] = x.disp;
		if (o->counts != nullptr)
			o->counts[i] = (uint16_t)x.count;
		for (uint32_t f = 0; f < x.count; ++f)
		{
			const uint8_t* from = b->data + b->offsets[i];
			uint32_t len = b->caplens[i];
			if (x.disp != PCPPX_FRAG_SPLIT)
			{
				if (o->data != nullptr && len != 0)
					std::memcpy(o->data + pos, from, len);
			}
			else
			{
				const uint32_t head = x.ip_off + x.hdr, gap = x.v6 ? 8u : 0u, piece = std::min(x.fs, x.pay - f * x.fs);
				len = head + gap + piece;
				if (o->data != nullptr)
				{
					uint8_t* d = o->data + pos;
					std::memcpy(d, from, head);
					std::memcpy(d + head + gap, from + head + (size_t)f * x.fs, piece);
					uint8_t* ip = d + x.ip_off;
					if (x.v6)
					{
						// the fragment header addExtension puts behind the last extension, and the payload length as
						// computeCalculateFields leaves it
						const uint32_t id = s->ids != nullptr ? s->ids[i] : s->id_base + i;
						const uint32_t word = (f * x.fs) | (f + 1 < x.count ? 1u : 0u), plen = x.hdr - 40 + 8 + piece;
						uint8_t* fh = d + head;
						fh[0] = d[x.nh_at];
						fh[1] = 0;
						fh[2] = (uint8_t)(word >> 8);
						fh[3] = (uint8_t)word;
						fh[4] = (uint8_t)(id >> 24);
						fh[5] = (uint8_t)(id >> 16);
						fh[6] = (uint8_t)(id >> 8);
						fh[7] = (uint8_t)id;
						d[x.nh_at] = 44;
						ip[4] = (uint8_t)(plen >> 8);
						ip[5] = (uint8_t)plen;
						// the type field ahead of a VLAN layer, as the layer in front of it recomputes it
						const uint32_t nl = std::min<uint32_t>(nlc[(size_t)i * stride], max_layers);
						const pcppx_layer* lay = &r->layers[(size_t)i * max_layers];
						for (uint32_t k = 0; k + 1 < nl && lay[k].proto != 3; ++k)
							if (lay[k + 1].proto == 9 && lay[k + 1].offset >= 2 && lay[k + 1].offset <= x.ip_off)
							{
								d[lay[k + 1].offset - 2] = 0x81;
								d[lay[k + 1].offset - 1] = 0x00;
							}
					}
					else
					{
						// the header as setIPv4FragmentParams and computeCalculateFields leave it
						const uint32_t tot_len = x.hdr + piece, word = (f * x.fs / 8) | (f + 1 < x.count ? 0x2000u : 0u);
						ip[2] = (uint8_t)(tot_len >> 8);
						ip[3] = (uint8_t)tot_len;
						ip[6] = (uint8_t)(word >> 8);
						ip[7] = (uint8_t)word;
						ip[10] = ip[11] = 0;
						uint32_t sum = 0;
						for (uint32_t k = 0; k < x.hdr; k += 2)
							sum += ((uint32_t)ip[k] << 8) | (k + 1 < x.hdr ? ip[k + 1] : 0u);
						while (sum >> 16)
							sum = (sum & 0xFFFFu) + (sum >> 16);
						ip[10] = (uint8_t)(~sum >> 8);
						ip[11] = (uint8_t)~sum;
					}
				}
			}
			o->offsets[j] = pos;
			o->caplens[j] = len;
			if (o->index != nullptr)
				o->index[j] = i;
			if (o->frag_no != nullptr)
				o->frag_no[j] = (uint16_t)f;
			++j;
			pos += len;
		}
	}
	return PCPPX_OK;
}
}  // namespace

extern "C"
{
	int pcppx_frag_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                      const pcppx_frag_spec* s, pcppx_fragmented* o, void* hip_stream)
	{
		pcppx_frag6_spec w;
		if (c == nullptr || !widen_frag_spec(s, w) || !valid_frag6(b, r, max_layers, &w, o))
			return PCPPX_E_INVAL;
		return frag_device(c, b, r, max_layers, &w, o, hip_stream);
	}

	int pcppx_frag_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_frag_spec* s,
	                         pcppx_fragmented* o)
	{
		pcppx_frag6_spec w;
		if (!widen_frag_spec(s, w) || !valid_frag6(b, r, max_layers, &w, o))
			return PCPPX_E_INVAL;
		return frag_reference(b, r, max_layers, &w, o);
	}

	int pcppx_frag6_device(pcppx_ctx* c, const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                       const pcppx_frag6_spec* s, pcppx_fragmented* o, void* hip_stream)
	{
		if (c == nullptr || !valid_frag6(b, r, max_layers, s, o))
			return PCPPX_E_INVAL;
		return frag_device(c, b, r, max_layers, s, o, hip_stream);
	}

	int pcppx_frag6_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
	                          const pcppx_frag6_spec* s, pcppx_fragmented* o)
	{
		if (!valid_frag6(b, r, max_layers, s, o))
			return PCPPX_E_INVAL;
		return frag_reference(b, r, max_layers, s, o);
	}
}

// ---- bpf: classic BPF programs over the packets of a batch (include/pcppx.h, bpf) ----
struct pcppx_bpf
{
	int device = 0;
	pcppx_bpf_insn* d_insns = nullptr;
	pcppx::BpfPrograms progs{};
	// recorded after every pcppx_bpf_device launch (on whatever stream): pcppx_bpf_free waits for it
	hipEvent_t used = nullptr;
	bool pending = false;
};

namespace
{
// the opcodes of the machine in include/pcppx.h (the BPF_* values of <pcap/bpf.h>)
enum : uint16_t
{
	kBpfLdW = 0x00, kBpfLdH = 0x08, kBpfLdB = 0x10,
	kBpfImm = 0x00, kBpfAbs = 0x20, kBpfInd = 0x40, kBpfMem = 0x60, kBpfLen = 0x80, kBpfMsh = 0xa0,
	kBpfLd = 0x00, kBpfLdx = 0x01, kBpfSt = 0x02, kBpfStx = 0x03, kBpfAlu = 0x04, kBpfJmp = 0x05, kBpfRet = 0x06,
	kBpfMisc = 0x07,
	kBpfK = 0x00, kBpfX = 0x08, kBpfA = 0x10,
	kBpfAdd = 0x00, kBpfSub = 0x10, kBpfMul = 0x20, kBpfDiv = 0x30, kBpfOr = 0x40, kBpfAnd = 0x50, kBpfLsh = 0x60,
	kBpfRsh = 0x70, kBpfNeg = 0x80, kBpfMod = 0x90, kBpfXor = 0xa0,
	kBpfJa = 0x00, kBpfJeq = 0x10, kBpfJgt = 0x20, kBpfJge = 0x30, kBpfJset = 0x40,
	kBpfTax = 0x00, kBpfTxa = 0x80,
};

bool bpf_is_ret(uint16_t code)
{
	return code == (kBpfRet | kBpfK) || code == (kBpfRet | kBpfA);
}

// one instruction at position i of n: a known opcode with legal operands
bool bpf_insn_ok(const pcppx_bpf_insn& in, uint32_t i, uint32_t n)
{
	const uint16_t c = in.code;
	switch (c)
	{
	case kBpfLd | kBpfLdW | kBpfAbs:
	case kBpfLd | kBpfLdH | kBpfAbs:
	case kBpfLd | kBpfLdB | kBpfAbs:
	case kBpfLd | kBpfLdW | kBpfInd:
	case kBpfLd | kBpfLdH | kBpfInd:
	case kBpfLd | kBpfLdB | kBpfInd:
	case kBpfLdx | kBpfLdB | kBpfMsh:
	case kBpfLd | kBpfImm:
	case kBpfLdx | kBpfImm:
	case kBpfLd | kBpfLdW | kBpfLen:
	case kBpfLdx | kBpfLdW | kBpfLen:
	case kBpfMisc | kBpfTax:
	case kBpfMisc | kBpfTxa:
	case kBpfAlu | kBpfNeg:
		return true;
	case kBpfLd | kBpfMem:
	case kBpfLdx | kBpfMem:
	case kBpfSt:
	case kBpfStx:
		return in.k < PCPPX_BPF_MEMWORDS;
	case kBpfJmp | kBpfJa:
		return in.k < n && (uint64_t)i + 1 + in.k < n;
	default:
		break;
	}
	if (bpf_is_ret(c))
		return true;
	const uint16_t cls = c & 0x07, src = c & 0x08, op = c & 0xf0;
	if ((c & ~0xffu) != 0)
		return false;
	if (cls == kBpfAlu)
	{
		switch (op)
		{
		case kBpfAdd:
		case kBpfSub:
		case kBpfMul:
		case kBpfOr:
		case kBpfAnd:
		case kBpfXor:
		case kBpfLsh:
		case kBpfRsh:
			return true;
		case kBpfDiv:
		case kBpfMod:
			return src == kBpfX || in.k != 0;
		default:
			return false;
		}
	}
	if (cls == kBpfJmp && (op == kBpfJeq || op == kBpfJgt || op == kBpfJge || op == kBpfJset))
		return (uint64_t)i + 1 + in.jt < n && (uint64_t)i + 1 + in.jf < n;
	return false;
}

int bpf_validate(const pcppx_bpf_insn* insns, uint32_t n)
{
	if (insns == nullptr || n < 1 || n > PCPPX_BPF_MAX_INSNS)
		return PCPPX_E_INVAL;
	for (uint32_t i = 0; i < n; ++i)
		if (!bpf_insn_ok(insns[i], i, n))
			return PCPPX_E_INVAL;
	return bpf_is_ret(insns[n - 1].code) ? PCPPX_OK : PCPPX_E_INVAL;
}

int bpf_validate_all(const pcppx_bpf_prog* progs, uint32_t n_progs)
{
	if (progs == nullptr || n_progs == 0 || n_progs > PCPPX_BPF_MAX_PROGRAMS)
		return PCPPX_E_INVAL;
	for (uint32_t q = 0; q < n_progs; ++q)
		if (progs[q].reserved != 0 || bpf_validate(progs[q].insns, progs[q].n_insns) != PCPPX_OK)
			return PCPPX_E_INVAL;
	return PCPPX_OK;
}

bool valid_bpf_io(const pcppx_batch* b, const pcppx_bpf_verdicts* o)
{
	if (b == nullptr || o == nullptr || o->totals == nullptr)
		return false;
	return valid_batch(b);
}

uint32_t bpf_be(const uint8_t* p, uint32_t size)
{
	uint32_t v = 0;
	for (uint32_t j = 0; j < size; ++j)
		v = (v << 8) | p[j];
	return v;
}

// one validated program over one packet: bpf_filter's result
uint32_t bpf_run(const pcppx_bpf_insn* insns, uint32_t n, const uint8_t* p, uint32_t buflen, uint32_t wirelen)
{
	uint32_t A = 0, X = 0, M[PCPPX_BPF_MEMWORDS] = {};
	for (uint32_t pc = 0; pc < n;)
	{
		const pcppx_bpf_insn& in = insns[pc++];
		const uint32_t k = in.k;
		const uint16_t c = in.code, cls = c & 0x07;
		if (cls == kBpfLd || cls == kBpfLdx)
		{
			const uint16_t mode = c & 0xe0;
			uint32_t v;
			if (mode == kBpfImm)
				v = k;
			else if (mode == kBpfMem)
				v = M[k];
			else if (mode == kBpfLen)
				v = wirelen;
			else
			{
				const uint32_t size = (c & 0x18) == kBpfLdW ? 4 : (c & 0x18) == kBpfLdH ? 2 : 1;
				const uint32_t x = mode == kBpfInd ? X : 0;
				if (k > buflen || x > buflen - k || size > buflen - (x + k))
					return 0;
				v = bpf_be(p + x + k, size);
				if (mode == kBpfMsh)
					v = (v & 0xf) << 2;
			}
			(cls == kBpfLdx ? X : A) = v;
		}
		else if (cls == kBpfSt)
			M[k] = A;
		else if (cls == kBpfStx)
			M[k] = X;
		else if (cls == kBpfAlu)
		{
			const uint32_t s = (c & 0x08) ? X : k;
			switch (c & 0xf0)
			{
			case kBpfAdd: A += s; break;
			case kBpfSub: A -= s; break;
			case kBpfMul: A *= s; break;
			case kBpfDiv:
				if (s == 0)
					return 0;
				A /= s;
				break;
			case kBpfMod:
				if (s == 0)
					return 0;
				A %= s;
				break;
			case kBpfOr: A |= s; break;
			case kBpfAnd: A &= s; break;
			case kBpfXor: A ^= s; break;
			case kBpfLsh: A = s < 32 ? A << s : 0; break;
			case kBpfRsh: A = s < 32 ? A >> s : 0; break;
			default: A = 0u - A; break;  // NEG
			}
		}
		else if (cls == kBpfJmp)
		{
			const uint32_t s = (c & 0x08) ? X : k;
			const uint16_t op = c & 0xf0;
			if (op == kBpfJa)
				pc += k;
			else
			{
				const bool t = op == kBpfJeq ? A == s : op == kBpfJgt ? A > s : op == kBpfJge ? A >= s : (A & s) != 0;
				pc += t ? in.jt : in.jf;
			}
		}
		else if (cls == kBpfRet)
			return (c & 0x18) == kBpfA ? A : k;
		else if ((c & 0xf8) == kBpfTxa)
			A = X;
		else
			X = A;
	}
	return 0;  // not reached by a validated program (its last instruction is a RET)
}
}  // namespace

extern "C"
{
	int pcppx_bpf_validate(const pcppx_bpf_insn* insns, uint32_t n_insns)
	{
		return bpf_validate(insns, n_insns);
	}

	int pcppx_bpf_load(pcppx_ctx* c, const pcppx_bpf_prog* progs, uint32_t n_progs, pcppx_bpf** out)
	{
		if (c == nullptr || out == nullptr || bpf_validate_all(progs, n_progs) != PCPPX_OK)
			return PCPPX_E_INVAL;
		*out = nullptr;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		pcppx_bpf* f = new (std::nothrow) pcppx_bpf;
		if (f == nullptr)
			return PCPPX_E_NOMEM;
		f->device = c->device;
		f->progs.n_progs = n_progs;
		std::vector<pcppx_bpf_insn> all;
		for (uint32_t q = 0; q < n_progs; ++q)
		{
			f->progs.start[q] = (uint32_t)all.size();
			for (uint32_t i = 0; i < progs[q].n_insns; ++i)
			{
				const pcppx_bpf_insn& in = progs[q].insns[i];
				if (in.code == (kBpfLd | kBpfMem) || in.code == (kBpfLdx | kBpfMem))
					f->progs.uses_mem |= 1u << q;
				all.push_back(in);
			}
		}
		for (uint32_t q = n_progs; q <= PCPPX_BPF_MAX_PROGRAMS; ++q)
			f->progs.start[q] = (uint32_t)all.size();
		int rc = PCPPX_OK;
		if (!ok(hipMalloc(reinterpret_cast<void**>(&f->d_insns), all.size() * sizeof(pcppx_bpf_insn))))
			rc = PCPPX_E_NOMEM;
		else if (!ok(hipMemcpy(f->d_insns, all.data(), all.size() * sizeof(pcppx_bpf_insn), hipMemcpyHostToDevice)) ||
		         !ok(hipEventCreateWithFlags(&f->used, hipEventDisableTiming)))
			rc = PCPPX_E_HIP;
		if (rc != PCPPX_OK)
		{
			pcppx_bpf_free(f);
			return rc;
		}
		f->progs.insns = f->d_insns;
		*out = f;
		return PCPPX_OK;
	}

	void pcppx_bpf_free(pcppx_bpf* f)
	{
		if (f == nullptr)
			return;
		(void)hipSetDevice(f->device);
		if (f->pending)
			(void)hipEventSynchronize(f->used);
		if (f->d_insns)
			(void)hipFree(f->d_insns);
		if (f->used)
			(void)hipEventDestroy(f->used);
		delete f;
	}

	int pcppx_bpf_device(pcppx_ctx* c, const pcppx_bpf* f, const pcppx_batch* b, const uint32_t* frame_lens,
	                     pcppx_bpf_verdicts* o, void* hip_stream)
	{
		if (c == nullptr || f == nullptr || !valid_bpf_io(b, o))
			return PCPPX_E_INVAL;
		if (f->device != c->device)
			return PCPPX_E_INVAL;
		if (!ok(hipSetDevice(c->device)))
			return PCPPX_E_HIP;
		hipStream_t st = static_cast<hipStream_t>(hip_stream);
		if (!ok(hipMemsetAsync(o->totals, 0, PCPPX_BPF_TOTALS * sizeof(uint64_t), st)))
			return PCPPX_E_HIP;
		if (b->n == 0)
			return PCPPX_OK;
		const int rc = pcppx::launch_bpf(b, frame_lens, f->progs, o, st);
		if (rc != PCPPX_OK)
			return rc;
		// the handle's own bookkeeping, not the programs: free waits for the last launch that reads them
		pcppx_bpf* h = const_cast<pcppx_bpf*>(f);
		if (!ok(hipEventRecord(h->used, st)))
			return PCPPX_E_HIP;
		h->pending = true;
		return PCPPX_OK;
	}

	int pcppx_bpf_reference(const pcppx_bpf_prog* progs, uint32_t n_progs, const pcppx_batch* b, const uint32_t* frame_lens,
	                        pcppx_bpf_verdicts* o)
	{
		if (bpf_validate_all(progs, n_progs) != PCPPX_OK || !valid_bpf_io(b, o))
			return PCPPX_E_INVAL;
		uint64_t n_matched = 0, n_bad = 0;
		for (uint32_t i = 0; i < b->n; ++i)
		{
			uint8_t matched = 0, bucket = 0xFF;
			uint32_t ret = 0;
			uint64_t off;
			uint32_t cap;
			if (out_of_bounds(b, 0, i, off, cap))
				++n_bad;
			else
			{
				const uint32_t wirelen = frame_lens != nullptr ? frame_lens[i] : cap;
				for (uint32_t q = 0; q < n_progs && !matched; ++q)
				{
					const uint32_t r = bpf_run(progs[q].insns, progs[q].n_insns, b->data + off, cap, wirelen);
					if (r != 0)
					{
						matched = 1;
						bucket = (uint8_t)q;
						ret = r;
					}
				}
				n_matched += matched;
			}
			if (o->matched != nullptr)
				o->matched[i] = matched;
			if (o->bucket != nullptr)
				o->bucket[i] = bucket;
			if (o->ret != nullptr)
				o->ret[i] = ret;
		}
		for (int k = 0; k < PCPPX_BPF_TOTALS; ++k)
			o->totals[k] = 0;
		o->totals[PCPPX_BPF_MATCHED] = n_matched;
		o->totals[PCPPX_BPF_BAD_DESC] = n_bad;
		return PCPPX_OK;
	}
}
