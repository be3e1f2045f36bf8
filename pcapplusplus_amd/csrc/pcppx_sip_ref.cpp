// pcppx_sip_ref.cpp — pcppx_sip_reference: the contract of pcppx_sip_device (include/pcppx.h, sip) in plain C++ over
// host pointers: one loop over the packets. No HIP: the file also builds with a host compiler alone (the sanitizer test
// of tests/test_sip.py does that). The dispatch, the first lines, the walk and the SDP body are pcppx_sip.h's, which the
// device kernels compile too; the independent restatement is pcapplusplus_amd/sip.py.
#include <cstring>
#include <vector>

#include "pcppx.h"
#include "pcppx_sip.h"

extern "C" int pcppx_sip_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                   const pcppx_sip_spec* s, pcppx_sip_out* o)
{
	using namespace pcppx::sip;
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
	std::vector<uint8_t> disp(n, PCPPX_SIP_NONE);
	uint64_t kinds[2] = { 0, 0 }, recs = 0, text = 0, host = 0, bad = 0, header = 0, linked = 0, sdps = 0, heur = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_SIP_BAD_DESC;
			++bad;
			continue;
		}
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		const Layer l =
		    find_layer(b->data + off, cap, r->layers + (size_t)i * max_layers, br.n_layers, max_layers, br.flags, s->kinds);
		disp[i] = (uint8_t)l.disp;
		host += l.disp == PCPPX_SIP_HOST;
		if (l.disp != PCPPX_SIP_MSG)
			continue;
		CountSink count;
		const Walk w = walk(b->data + off + l.off, l, s, count);
		found.push_back({ i, l });
		++kinds[l.kind];
		recs += w.n_rec;
		text += w.text_len;
		header += w.header_len;
		linked += w.n_fields;
		sdps += (w.flags & PCPPX_SIP_HAS_SDP) != 0;
		heur += l.via;
	}
	for (int k = 0; k < PCPPX_SIP_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_SIP_MSGS] = found.size();
	o->totals[PCPPX_SIP_REQUESTS] = kinds[0];
	o->totals[PCPPX_SIP_RESPONSES] = kinds[1];
	o->totals[PCPPX_SIP_FIELDS] = recs;
	o->totals[PCPPX_SIP_TEXT_BYTES] = text;
	o->totals[PCPPX_SIP_HOST_N] = host;
	o->totals[PCPPX_SIP_BAD_DESC_N] = bad;
	o->totals[PCPPX_SIP_HEADER_BYTES] = header;
	o->totals[PCPPX_SIP_FIELDS_LINKED] = linked;
	o->totals[PCPPX_SIP_SDPS] = sdps;
	o->totals[PCPPX_SIP_BY_HEURISTIC] = heur;
	if (found.size() > o->max_msgs || found.size() > (s->max_msgs == 0 ? n : s->max_msgs) || recs > o->max_fields ||
	    sdps > o->max_sdps || (o->text != nullptr && text > o->text_cap))
	{
		o->totals[PCPPX_SIP_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	if (o->disposition != nullptr)
		for (uint32_t i = 0; i < n; ++i)
			o->disposition[i] = disp[i];
	uint64_t first_field = 0, pos = 0, sdp = 0;
	for (size_t j = 0; j < found.size(); ++j)
	{
		const Found& f = found[j];
		const uint8_t* d = b->data + b->offsets[f.index] + f.l.off;
		EmitSink sink{ o->fields + first_field, o->text, pos, (uint32_t)j };
		const Walk w = walk(d, f.l, s, sink);
		if ((w.flags & PCPPX_SIP_HAS_SDP) != 0)
		{
			const Sdp x = sdp_of(d + w.header_len, f.l.L - w.header_len);
			put_sdp(o->sdps + sdp++, (uint32_t)j, f.index, w.header_len, f.l.L - w.header_len, x);
		}
		put_msg(o->msgs + j, first_field, pos, f.index, f.l, w);
		first_field += w.n_rec;
		pos += w.text_len;
	}
	return PCPPX_OK;
}
