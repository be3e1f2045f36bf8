// pcppx_tcpstream_ref.cpp — pcppx_tcpstream_reference: the contract of pcppx_tcpstream_device (include/pcppx.h, tcpstream)
// in plain C++ over host pointers: group, sort and walk. No HIP: the file also builds with a host compiler alone (the
// sanitizer test of tests/test_tcpstream.py does that).
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "pcppx.h"

namespace pcppx
{
// the argument rules pcppx_tcpstream_device and pcppx_tcpstream_reference share (include/pcppx.h)
bool valid_tcpstream(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_reasm_info* info,
                     const pcppx_tcpstream_spec* s, const pcppx_tcpstreams* o)
{
	if (b == nullptr || r == nullptr || s == nullptr || o == nullptr || o->totals == nullptr || o->streams == nullptr)
		return false;
	if (max_layers == 0 || max_layers > PCPPX_MAX_LAYERS || r->layout != PCPPX_LAYOUT_FIXED)
		return false;
	if (s->base_clear > 1 || s->reserved[0] != 0 || s->reserved[1] != 0 || s->reserved[2] != 0 || o->reserved != 0)
		return false;
	if (b->n != 0 && (info == nullptr || r->layers == nullptr || (r->summary == nullptr && r->brief == nullptr)))
		return false;
	return b->n == 0 || (b->offsets != nullptr && b->caplens != nullptr && (b->data != nullptr || b->data_len == 0));
}
}  // namespace pcppx

namespace
{
struct Seg
{
	uint32_t idx, seq, len, pay, rel;
	uint8_t st;
	std::array<uint8_t, 19> src;  // family, the raw port bytes, the address
};

struct Side
{
	std::vector<Seg> members;  // in source order
	bool clean = false, in_order = true;
	uint64_t bytes = 0;
	uint32_t n_data = 0, flags = 0, rank = PCPPX_TCPS_NONE;
	uint64_t pos = 0;
};
}  // namespace

extern "C" int pcppx_tcpstream_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                         const pcppx_reasm_info* info, const pcppx_tcpstream_spec* s,
                                         pcppx_tcpstreams* o)
{
	if (!pcppx::valid_tcpstream(b, r, max_layers, info, s, o))
		return PCPPX_E_INVAL;
	const uint32_t n = b->n;
	std::vector<uint8_t> disp(n, PCPPX_TCPS_NOT_TCP);
	std::map<uint32_t, std::vector<Seg>> conns;  // the candidates by hash5, in source order
	uint64_t candidates = 0, bad = 0, host = 0;
	const uint8_t* rec0 = nullptr;
	size_t stride = 0;
	if (n != 0)
	{
		rec0 = r->summary != nullptr ? reinterpret_cast<const uint8_t*>(r->summary) : reinterpret_cast<const uint8_t*>(r->brief);
		stride = r->summary != nullptr ? sizeof(pcppx_summary) : sizeof(pcppx_brief);
	}
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_TCPS_BAD_DESC;
			++bad;
			continue;
		}
		const uint8_t st = info[i].tcp_status;
		if ((st & 15) == PCPPX_TCPR_HOST)
		{
			disp[i] = PCPPX_TCPS_HOST;
			++host;
			continue;
		}
		if ((st & 15) != PCPPX_TCPR_DATA)
			continue;
		disp[i] = PCPPX_TCPS_LEFT;  // until its side turns out clean
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		const uint32_t nl = std::min<uint32_t>(br.n_layers, max_layers);
		if (br.l4_layer >= nl)
			continue;
		const pcppx_layer* lay = r->layers + (size_t)i * max_layers;
		const pcppx_layer& T = lay[br.l4_layer];
		if (T.proto != 4 || (uint32_t)T.offset + 20 > cap || (uint64_t)T.offset + T.hdr_len + info[i].tcp_payload > cap)
			continue;
		uint32_t fam = 0, ip_off = 0;
		for (uint32_t k = 0; k < nl && fam == 0; ++k)
			if (lay[k].proto == 2 || lay[k].proto == 3)  // pcpp::IPv4 / IPv6: the first IP layer
			{
				fam = lay[k].proto == 2 ? 4 : 6;
				ip_off = lay[k].offset;
			}
		if (fam == 0 || ip_off + (fam == 4 ? 16u : 24u) > cap)
			continue;
		const uint8_t* pk = b->data + off;
		const uint8_t* t = pk + T.offset;
		Seg g{};
		g.idx = i;
		g.seq = ((uint32_t)t[4] << 24) | ((uint32_t)t[5] << 16) | ((uint32_t)t[6] << 8) | t[7];
		g.len = info[i].tcp_payload;
		g.pay = (uint32_t)T.offset + T.hdr_len;
		g.st = st;
		g.src.fill(0);
		g.src[0] = (uint8_t)fam;
		g.src[1] = t[0];
		g.src[2] = t[1];
		std::memcpy(&g.src[3], pk + ip_off + (fam == 4 ? 12 : 8), fam == 4 ? 4 : 16);
		conns[br.hash5].push_back(g);
		++candidates;
	}
	for (int k = 0; k < PCPPX_TCPS_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_TCPS_CANDIDATES] = candidates;
	o->totals[PCPPX_TCPS_HOST_N] = host;
	o->totals[PCPPX_TCPS_BAD_DESC_N] = bad;
	if (candidates > (s->max_segments == 0 ? n : s->max_segments))  // no room to form the connections
	{
		o->totals[PCPPX_TCPS_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	// the sides, judged one by one; the clean ones keyed by their first member's source index
	std::map<uint32_t, std::pair<uint32_t, Side*>> clean;  // first -> (hash5, side)
	std::map<uint32_t, std::array<Side, 2>> sides;
	for (auto& kv : conns)
	{
		std::array<Side, 2>& sd = sides[kv.first];
		const std::vector<Seg>& all = kv.second;
		for (const Seg& g : all)
		{
			if (g.src == all[0].src)
				sd[0].members.push_back(g);
			else if (sd[1].members.empty() || g.src == sd[1].members[0].src)
				sd[1].members.push_back(g);
			// else a third source: LEFT
		}
		uint32_t min_rst = 0xFFFFFFFFu, last_data = 0;
		for (Side& x : sd)
			for (Seg& g : x.members)
			{
				const Seg& f = x.members[0];
				g.rel = g.seq - (f.seq + ((f.st & PCPPX_TCPR_F_SYN) ? 1u : 0u));
				if (g.st & PCPPX_TCPR_F_RST)
					min_rst = std::min(min_rst, g.idx);
				if (g.len > 0)
					last_data = std::max(last_data, g.idx);
			}
		size_t later_data[2] = { 0, 0 };  // a side's data members besides its own first member
		for (int d = 0; d < 2; ++d)
			for (size_t k = 1; k < sd[d].members.size(); ++k)
				later_data[d] += sd[d].members[k].len > 0;
		for (int d = 0; d < 2; ++d)
		{
			Side& x = sd[d];
			if (x.members.empty())
				continue;
			bool ok = true;
			uint32_t min_fin = 0xFFFFFFFFu, my_last = 0;
			std::vector<Seg> data;
			for (const Seg& g : x.members)
			{
				x.flags |= ((g.st & PCPPX_TCPR_F_SYN) ? PCPPX_TCPS_F_SYN : 0) | ((g.st & PCPPX_TCPR_F_FIN) ? PCPPX_TCPS_F_FIN : 0) |
				           ((g.st & PCPPX_TCPR_F_RST) ? PCPPX_TCPS_F_RST : 0);
				if (g.st & (PCPPX_TCPR_F_FIN | PCPPX_TCPR_F_RST))
					min_fin = std::min(min_fin, g.idx);
				if (g.len == 0)
					continue;
				ok = ok && (g.st & PCPPX_TCPR_F_SYN) == 0 && g.rel < 0x80000000u;  // 1, 2
				my_last = std::max(my_last, g.idx);
				if (!data.empty() && g.rel < data.back().rel)
					x.in_order = false;
				data.push_back(g);
			}
			ok = ok && !data.empty();  // 6
			std::stable_sort(data.begin(), data.end(), [](const Seg& p, const Seg& q) { return p.rel < q.rel; });
			uint64_t at = 0;
			for (const Seg& g : data)
			{
				ok = ok && g.rel == at;  // 2: the exact tiling
				at += g.len;
			}
			ok = ok && at < 0x80000000ull;
			ok = ok && min_fin >= my_last;   // 3
			ok = ok && min_rst >= last_data;  // 4
			const size_t other = later_data[1 - d];
			ok = ok && (s->base_clear == 0 || x.in_order || other == 0);  // 5
			x.clean = ok;
			x.bytes = at;
			x.n_data = (uint32_t)data.size();
			if (!x.in_order)
				x.flags |= PCPPX_TCPS_F_OOO;
			if (ok)
			{
				std::vector<Seg> ordered = data;  // the data members in rel order, then the control members
				for (const Seg& g : x.members)
					if (g.len == 0)
						ordered.push_back(g);
				for (const Seg& g : ordered)
					disp[g.idx] = g.len > 0 ? PCPPX_TCPS_STREAM : PCPPX_TCPS_CONTROL;
				clean[x.members[0].idx] = { kv.first, &x };
				x.members.swap(ordered);
			}
		}
	}
	uint64_t n_streams = 0, bytes = 0, segments = 0, left = 0;
	for (auto& kv : clean)
	{
		Side& x = *kv.second.second;
		x.rank = (uint32_t)n_streams++;
		x.pos = bytes;
		bytes += x.bytes;
		segments += x.n_data;
	}
	for (uint32_t i = 0; i < n; ++i)
		left += disp[i] == PCPPX_TCPS_LEFT;
	const bool overflow = n_streams > o->max_streams || (o->data != nullptr && bytes > o->data_cap);
	o->totals[PCPPX_TCPS_STREAMS] = n_streams;
	o->totals[PCPPX_TCPS_BYTES] = bytes;
	o->totals[PCPPX_TCPS_SEGMENTS] = segments;
	o->totals[PCPPX_TCPS_LEFT_N] = left;
	o->totals[PCPPX_TCPS_OVERFLOW] = overflow ? 1 : 0;
	if (overflow)
		return PCPPX_OK;
	for (uint32_t i = 0; i < n; ++i)
	{
		if (o->disposition != nullptr)
			o->disposition[i] = disp[i];
		if (o->seg_stream != nullptr)
			o->seg_stream[i] = PCPPX_TCPS_NONE;
		if (o->seg_pos != nullptr)
			o->seg_pos[i] = 0;
	}
	for (auto& kv : clean)
	{
		const uint32_t key = kv.second.first;
		const Side& x = *kv.second.second;
		std::array<Side, 2>& sd = sides[key];
		const int d = &x == &sd[1] ? 1 : 0;
		pcppx_tcpstream_rec rec{};
		rec.pos = x.pos;
		rec.bytes = (uint32_t)x.bytes;
		rec.flow_key = key;
		rec.first = kv.first;
		rec.segments = x.n_data;
		rec.peer = sd[1 - d].clean ? sd[1 - d].rank : PCPPX_TCPS_NONE;
		rec.side = (uint8_t)d;
		rec.flags = (uint8_t)x.flags;
		o->streams[x.rank] = rec;
		for (const Seg& g : x.members)  // the data members in rel order, then the control members
		{
			if (o->seg_stream != nullptr)
				o->seg_stream[g.idx] = x.rank;
			if (o->seg_pos != nullptr)
				o->seg_pos[g.idx] = g.rel;
			if (o->data != nullptr && g.len > 0)
				std::memcpy(o->data + x.pos + g.rel, b->data + b->offsets[g.idx] + g.pay, g.len);
		}
	}
	return PCPPX_OK;
}
