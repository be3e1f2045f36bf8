// pcppx_dhcp_ref.cpp — pcppx_dhcp_reference: the contract of pcppx_dhcp_device (include/pcppx.h, dhcp) in plain C++
// over host pointers: one loop over the packets. No HIP: the file also builds with a host compiler alone (the sanitizer
// test of tests/test_dhcp.py does that). The dispatch, the walks and the typed values are pcppx_dhcp.h's, which the
// device kernels compile too; the independent restatement is pcapplusplus_amd/dhcp.py.
#include <cstring>
#include <vector>

#include "pcppx.h"
#include "pcppx_dhcp.h"

static_assert(sizeof(pcppx_dhcp_spec) == 72 && sizeof(pcppx_dhcp_option) == 16 && sizeof(pcppx_dhcp_msg) == 80 &&
                  sizeof(pcppx_dhcp_out) == 64,
              "include/pcppx.h");

extern "C" int pcppx_dhcp_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                    const pcppx_dhcp_spec* s, pcppx_dhcp_out* o)
{
	using namespace pcppx::dhcp;
	if (!valid_args(b, r, max_layers, s, o))
		return PCPPX_E_INVAL;
	const uint32_t n = b->n;
	const uint8_t* rec0 = nullptr;
	size_t stride = 0;
	if (n != 0)
	{
		rec0 = r->summary != nullptr ? reinterpret_cast<const uint8_t*>(r->summary)
		                             : reinterpret_cast<const uint8_t*>(r->brief);
		stride = r->summary != nullptr ? sizeof(pcppx_summary) : sizeof(pcppx_brief);
	}
	struct Found
	{
		uint32_t index;
		Layer l;
	};
	std::vector<Found> found;
	std::vector<uint8_t> disp(n, PCPPX_DHCP_NONE);
	uint64_t fam[2] = { 0, 0 }, recs = 0, bytes = 0, host = 0, bad = 0, linked = 0, replies = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_DHCP_BAD_DESC;
			++bad;
			continue;
		}
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		const Layer l = find_layer(b->data + off, cap, r->layers + (size_t)i * max_layers, br.n_layers, max_layers,
		                           br.flags, s->families);
		disp[i] = (uint8_t)l.disp;
		host += l.disp == PCPPX_DHCP_HOST;
		if (l.disp != PCPPX_DHCP_MSG)
			continue;
		const uint8_t* d = b->data + off + l.off;
		CountSink count;
		const Walk w = walk(d, l.L, l.family, s, count);
		found.push_back({ i, l });
		++fam[l.family == 6];
		recs += w.n_rec;
		bytes += w.value_len;
		linked += w.n_options;
		replies += is_reply(d, l.family);
	}
	for (int k = 0; k < PCPPX_DHCP_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_DHCP_MSGS] = found.size();
	o->totals[PCPPX_DHCP_V4_N] = fam[0];
	o->totals[PCPPX_DHCP_V6_N] = fam[1];
	o->totals[PCPPX_DHCP_OPTIONS] = recs;
	o->totals[PCPPX_DHCP_VALUE_BYTES] = bytes;
	o->totals[PCPPX_DHCP_HOST_N] = host;
	o->totals[PCPPX_DHCP_BAD_DESC_N] = bad;
	o->totals[PCPPX_DHCP_OPTIONS_LINKED] = linked;
	o->totals[PCPPX_DHCP_REPLIES] = replies;
	if (found.size() > o->max_msgs || found.size() > (s->max_msgs == 0 ? n : s->max_msgs) || recs > o->max_options ||
	    (o->values != nullptr && bytes > o->values_cap))
	{
		o->totals[PCPPX_DHCP_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	if (o->disposition != nullptr)
		for (uint32_t i = 0; i < n; ++i)
			o->disposition[i] = disp[i];
	uint64_t first_option = 0, pos = 0;
	for (size_t j = 0; j < found.size(); ++j)
	{
		const Found& f = found[j];
		const uint8_t* d = b->data + b->offsets[f.index] + f.l.off;
		EmitSink sink{ o->options + first_option, o->values, pos, (uint32_t)j };
		const Walk w = walk(d, f.l.L, f.l.family, s, sink);
		put_msg(o->msgs + j, first_option, pos, f.index, d, f.l, w);
		first_option += w.n_rec;
		pos += w.value_len;
	}
	return PCPPX_OK;
}
