// pcppx_ssl_ref.cpp — pcppx_ssl_reference: the contract of pcppx_ssl_device (include/pcppx.h, ssl) in plain C++ over
// host pointers: one loop over the packets. No HIP: the file also builds with a host compiler alone (the sanitizer test
// of tests/test_ssl.py does that). The chain rule, the entry walk, the handshake walk and the hello records are
// pcppx_ssl.h's, which the device kernels compile too; the independent restatement is pcapplusplus_amd/ssl.py.
#include <cstring>
#include <vector>

#include "pcppx.h"
#include "pcppx_ssl.h"

extern "C" int pcppx_ssl_reference(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers,
                                   const pcppx_ssl_spec* s, pcppx_ssl_out* o)
{
	using namespace pcppx::ssl;
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
	std::vector<uint32_t> found;
	std::vector<uint8_t> disp(n, PCPPX_SSL_NONE);
	uint64_t hellos = 0, client = 0, names = 0, host = 0, bad = 0, payload = 0, alert = 0, appdata = 0;
	auto walk_packet = [&](uint32_t i, auto& sink) {
		pcppx_brief br;
		std::memcpy(&br, rec0 + (size_t)i * stride, sizeof br);
		return walk(b->data + b->offsets[i], b->caplens[i], r->layers + (size_t)i * max_layers, br.n_layers, max_layers,
		            br.flags, s->kinds, sink);
	};
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint64_t off = b->offsets[i];
		const uint32_t cap = b->caplens[i];
		if (off + cap < off || off + cap > b->data_len)
		{
			disp[i] = PCPPX_SSL_BAD_DESC;
			++bad;
			continue;
		}
		CountSink count;
		const Pkt w = walk_packet(i, count);
		disp[i] = (uint8_t)w.disp;
		host += w.disp == PCPPX_SSL_HOST;
		if (w.disp != PCPPX_SSL_MSG)
			continue;
		found.push_back(i);
		hellos += count.n_hellos;
		client += count.n_client;
		names += count.name_bytes;
		payload += w.payload_len;
		alert += type_count(w, kAlert) != 0;
		appdata += type_count(w, kAppData) != 0;
	}
	for (int k = 0; k < PCPPX_SSL_TOTALS; ++k)
		o->totals[k] = 0;
	o->totals[PCPPX_SSL_MSGS] = found.size();
	o->totals[PCPPX_SSL_HELLOS] = hellos;
	o->totals[PCPPX_SSL_CLIENT_HELLOS] = client;
	o->totals[PCPPX_SSL_SERVER_HELLOS] = hellos - client;
	o->totals[PCPPX_SSL_NAME_BYTES] = names;
	o->totals[PCPPX_SSL_HOST_N] = host;
	o->totals[PCPPX_SSL_BAD_DESC_N] = bad;
	o->totals[PCPPX_SSL_PAYLOAD_BYTES] = payload;
	o->totals[PCPPX_SSL_ALERT_PKTS] = alert;
	o->totals[PCPPX_SSL_APPDATA_PKTS] = appdata;
	if (found.size() > o->max_msgs || found.size() > (s->max_msgs == 0 ? n : s->max_msgs) || hellos > o->max_hellos ||
	    (o->names != nullptr && names > o->names_cap))
	{
		o->totals[PCPPX_SSL_OVERFLOW] = 1;
		return PCPPX_OK;
	}
	if (o->disposition != nullptr)
		for (uint32_t i = 0; i < n; ++i)
			o->disposition[i] = disp[i];
	uint64_t first_hello = 0, pos = 0;
	for (size_t j = 0; j < found.size(); ++j)
	{
		EmitSink sink{ o->hellos + first_hello, o->names, pos, (uint32_t)j };
		const Pkt w = walk_packet(found[j], sink);
		put_msg(o->msgs + j, first_hello, found[j], w, sink.n_hellos, sink.name_bytes);
		first_hello += sink.n_hellos;
		pos += sink.name_bytes;
	}
	return PCPPX_OK;
}
