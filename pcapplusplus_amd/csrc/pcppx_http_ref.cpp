// pcppx_http_ref.cpp — pcppx_http_reference: the contract of pcppx_http_device (include/pcppx.h, http) in plain C++
// over host pointers: one loop over the packets. No HIP: the file also builds with a host compiler alone (the sanitizer
// test of tests/test_http.py does that). The layer rule, the first lines and the walk are pcppx_http.h's, which the
// device kernels compile too; the independent restatement is pcapplusplus_amd/http.py.
#include <cstring>
#include <vector>

#include "pcppx.h"
#include "pcppx_http.h"

extern "C" int pcppx_http_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                    const pcppx_http_spec* s, pcppx_http_out* o)
{
	using namespace pcppx::http;
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
	std::vector<uint8_t> disp(n, PCPPX_HTTP_NONE);
	uint64_t kinds[2] = { 0, 0 }, recs = 0, text = 0, host = 0, bad = 0, header = 0, linked = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_HTTP_BAD_DESC;
			++bad;
			continue;
		}
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		const Layer l = find_layer(cap, r->layers + (size_t)i * max_layers, br.n_layers, max_layers, br.flags, s->kinds);
		disp[i] = (uint8_t)l.disp;
		host += l.disp == PCPPX_HTTP_HOST;
		if (l.disp != PCPPX_HTTP_MSG)
			continue;
		CountSink count;
		const Walk w = walk(b->data + off + l.off, l.L, l.kind, s, count);
		found.push_back({ i, l });
		++kinds[l.kind];
		recs += w.n_rec;
		text += w.text_len;
		header += w.header_len;
		linked += w.n_fields;
	}
	for (int k = 0; k < PCPPX_HTTP_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_HTTP_MSGS] = found.size();
	o->totals[PCPPX_HTTP_REQUESTS] = kinds[0];
	o->totals[PCPPX_HTTP_RESPONSES] = kinds[1];
	o->totals[PCPPX_HTTP_FIELDS] = recs;
	o->totals[PCPPX_HTTP_TEXT_BYTES] = text;
	o->totals[PCPPX_HTTP_HOST_N] = host;
	o->totals[PCPPX_HTTP_BAD_DESC_N] = bad;
	o->totals[PCPPX_HTTP_HEADER_BYTES] = header;
	o->totals[PCPPX_HTTP_FIELDS_LINKED] = linked;
	if (found.size() > o->max_msgs || found.size() > (s->max_msgs == 0 ? n : s->max_msgs) || recs > o->max_fields ||
	    (o->text != nullptr && text > o->text_cap))
	{
		o->totals[PCPPX_HTTP_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	if (o->disposition != nullptr)
		for (uint32_t i = 0; i < n; ++i)
			o->disposition[i] = disp[i];
	uint64_t first_field = 0, pos = 0;
	for (size_t j = 0; j < found.size(); ++j)
	{
		const Found& f = found[j];
		const uint8_t* d = b->data + b->offsets[f.index] + f.l.off;
		EmitSink sink{ o->fields + first_field, o->text, pos, (uint32_t)j };
		const Walk w = walk(d, f.l.L, f.l.kind, s, sink);
		put_msg(o->msgs + j, first_field, pos, f.index, f.l, w);
		first_field += w.n_rec;
		pos += w.text_len;
	}
	return PCPPX_OK;
}
