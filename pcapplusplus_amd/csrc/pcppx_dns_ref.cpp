// pcppx_dns_ref.cpp — pcppx_dns_reference: the contract of pcppx_dns_device (include/pcppx.h, dns) in plain C++ over
// host pointers: one loop over the packets. No HIP: the file also builds with a host compiler alone (the sanitizer
// test of tests/test_dns.py does that). The layer rule, the walk and the name decode are pcppx_dns.h's, which the
// device kernels compile too; the independent restatement is pcapplusplus_amd/dns.py.
#include <cstring>
#include <vector>

#include "pcppx.h"
#include "pcppx_dns.h"

extern "C" int pcppx_dns_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                   const pcppx_dns_spec* s, pcppx_dns_out* o)
{
	using namespace pcppx::dns;
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
		Walk w;
	};
	std::vector<Found> found;
	std::vector<uint8_t> disp(n, PCPPX_DNS_NONE);
	uint64_t rrs = 0, name_bytes = 0, host = 0, bad = 0, qa = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_DNS_BAD_DESC;
			++bad;
			continue;
		}
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		const Layer l = find_layer(cap, r->layers + (size_t)i * max_layers, br.n_layers, max_layers, br.flags);
		disp[i] = (uint8_t)l.disp;
		host += l.disp == PCPPX_DNS_HOST;
		if (l.disp != PCPPX_DNS_MSG)
			continue;
		CountSink count;
		const Walk w = walk(b->data + off + l.off, l.L, l.adj, s->sections, count);
		found.push_back({ i, l, w });
		rrs += w.n_rr;
		name_bytes += w.name_bytes;
		qa += count_of(w.linked, 0) + count_of(w.linked, 1);
	}
	for (int k = 0; k < PCPPX_DNS_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_DNS_MSGS] = found.size();
	o->totals[PCPPX_DNS_RRS] = rrs;
	o->totals[PCPPX_DNS_NAME_BYTES] = name_bytes;
	o->totals[PCPPX_DNS_HOST_N] = host;
	o->totals[PCPPX_DNS_BAD_DESC_N] = bad;
	o->totals[PCPPX_DNS_QA_LINKED] = qa;
	if (found.size() > o->max_msgs || found.size() > (s->max_msgs == 0 ? n : s->max_msgs) || rrs > o->max_rrs ||
	    (o->names != nullptr && name_bytes > o->names_cap))
	{
		o->totals[PCPPX_DNS_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	if (o->disposition != nullptr)
		for (uint32_t i = 0; i < n; ++i)
			o->disposition[i] = disp[i];
	uint64_t first_rr = 0, pos = 0;
	for (size_t j = 0; j < found.size(); ++j)
	{
		const Found& f = found[j];
		const uint8_t* d = b->data + b->offsets[f.index] + f.l.off;
		EmitSink sink{ o->rrs + first_rr, o->names, pos, (uint32_t)j };
		const Walk w = walk(d, f.l.L, f.l.adj, s->sections, sink);
		put_msg(o->msgs + j, first_rr, f.index, f.l, d, w);
		first_rr += w.n_rr;
		pos += w.name_bytes;
	}
	return PCPPX_OK;
}
