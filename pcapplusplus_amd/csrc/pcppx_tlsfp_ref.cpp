// pcppx_tlsfp_ref.cpp — pcppx_tlsfp_reference: the contract of pcppx_tlsfp_device (include/pcppx.h, tlsfp) in plain
// C++ over host pointers: one loop over the packets. No HIP: the file also builds with a host compiler alone (the
// sanitizer test of tests/test_tlsfp.py does that). The walk and the MD5 are pcppx_tlsfp.h's, which the device kernels
// compile too; the independent restatement is pcapplusplus_amd/tlsfp.py.
#include <cstring>
#include <vector>

#include "pcppx.h"
#include "pcppx_tlsfp.h"

extern "C" int pcppx_tlsfp_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                     const pcppx_tlsfp_spec* s, pcppx_tlsfps* o)
{
	using namespace pcppx::tlsfp;
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
		uint32_t index, text_len;
		Hello h;
	};
	std::vector<Found> found;
	std::vector<uint8_t> disp(n, PCPPX_TLSFP_NONE);
	uint64_t clients = 0, servers = 0, text_bytes = 0, host = 0, bad = 0;
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_TLSFP_BAD_DESC;
			++bad;
			continue;
		}
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		const uint8_t* pk = b->data + off;
		const Hello h = find_hello(pk, cap, r->layers + (size_t)i * max_layers, br.n_layers, max_layers, br.flags,
		                           s->client != 0, s->server != 0);
		disp[i] = (uint8_t)h.disp;
		host += h.disp == PCPPX_TLSFP_HOST;
		if (h.disp != PCPPX_TLSFP_CLIENT && h.disp != PCPPX_TLSFP_SERVER)
			continue;
		CountSink count;
		hello_text(pk + h.msg_off, h.D, h.M, h.disp, count);
		found.push_back({ i, count.len, h });
		(h.disp == PCPPX_TLSFP_CLIENT ? clients : servers) += 1;
		text_bytes += count.len;
	}
	for (int k = 0; k < PCPPX_TLSFP_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_TLSFP_HOST_N] = host;
	o->totals[PCPPX_TLSFP_BAD_DESC_N] = bad;
	o->totals[PCPPX_TLSFP_CANDIDATES] = found.size();
	if (found.size() > (s->max_hellos == 0 ? n : s->max_hellos))
	{
		o->totals[PCPPX_TLSFP_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	o->totals[PCPPX_TLSFP_CLIENT_N] = clients;
	o->totals[PCPPX_TLSFP_SERVER_N] = servers;
	o->totals[PCPPX_TLSFP_TEXT_BYTES] = text_bytes;
	if (found.size() > o->max_recs || (o->text != nullptr && text_bytes > o->text_cap))
	{
		o->totals[PCPPX_TLSFP_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	if (o->disposition != nullptr)
		for (uint32_t i = 0; i < n; ++i)
			o->disposition[i] = disp[i];
	uint64_t pos = 0;
	for (size_t j = 0; j < found.size(); ++j)
	{
		const Found& f = found[j];
		uint32_t block[16], digest[4];
		Md5Sink<1> sink(block, o->text != nullptr ? o->text + pos : nullptr);
		hello_text(b->data + b->offsets[f.index] + f.h.msg_off, f.h.D, f.h.M, f.h.disp, sink);
		sink.finish(digest);
		pcppx_tlsfp_rec rec;
		std::memset(&rec, 0, sizeof rec);
		for (int k = 0; k < 16; ++k)
			rec.md5[k] = (uint8_t)(digest[k >> 2] >> (8 * (k & 3)));
		rec.text_pos = pos;
		rec.text_len = f.text_len;
		rec.index = f.index;
		rec.msg_offset = (uint16_t)f.h.msg_off;
		rec.kind = (uint8_t)f.h.disp;
		o->recs[j] = rec;
		pos += f.text_len;
	}
	return PCPPX_OK;
}
