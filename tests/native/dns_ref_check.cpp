// dns_ref_check — pcppx_dns_reference on cases written by tests/test_dns.py, for a sanitizer build (host compiler, no
// HIP): dns_ref_check <file>...
// A .case file: 14 u64 words (n, data_len, max_layers, summary?, sections, the spec's max_msgs, out max_msgs, max_rrs,
// names_cap, names?, disposition?, message bytes, record bytes, name bytes), then the arrays: data, offsets, caplens,
// records, layers, and the expected messages, records, names, disposition and totals (every buffer whole, fill
// included).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcppx.h"

namespace
{
bool read(FILE* f, void* p, size_t bytes)
{
	return bytes == 0 || std::fread(p, 1, bytes, f) == bytes;
}

template <typename T>
bool load(FILE* f, std::vector<T>& v, size_t count)
{
	v.resize(count);
	return read(f, v.data(), count * sizeof(T));
}

int run(const char* path)
{
	FILE* f = std::fopen(path, "rb");
	if (f == nullptr)
		return 2;
	uint64_t h[14];
	if (!read(f, h, sizeof h))
		return 2;
	const uint64_t n = h[0], ml = h[2], msg_bytes = h[11], rr_bytes = h[12], name_bytes = h[13];
	const bool summary = h[3] != 0, has_names = h[9] != 0, has_disp = h[10] != 0;
	std::vector<uint8_t> data, rec, want_msgs, want_rrs, want_names, want_disp;
	std::vector<uint64_t> offsets, want_totals;
	std::vector<uint32_t> caplens;
	std::vector<pcppx_layer> layers;
	const size_t disp_n = has_disp ? n + 4 : 0;
	bool ok = load(f, data, h[1]) && load(f, offsets, n) && load(f, caplens, n) &&
	          load(f, rec, n * (summary ? sizeof(pcppx_summary) : sizeof(pcppx_brief))) && load(f, layers, n * ml) &&
	          load(f, want_msgs, msg_bytes) && load(f, want_rrs, rr_bytes) &&
	          load(f, want_names, has_names ? name_bytes : 0) && load(f, want_disp, disp_n) &&
	          load(f, want_totals, PCPPX_DNS_TOTALS);
	std::fclose(f);
	if (!ok)
		return 2;
	// exact-size heap buffers: a byte read or written past any of them is the sanitizer's to report
	std::vector<uint8_t> got_names(has_names ? name_bytes : 0, 0xA5), got_disp(disp_n, 0xA5);
	// (one entry where the case has room for none: a null out->msgs or out->rrs is refused)
	std::vector<pcppx_dns_msg> got_msgs(msg_bytes != 0 ? msg_bytes / sizeof(pcppx_dns_msg) : 1);
	std::vector<pcppx_dns_rr> got_rrs(rr_bytes != 0 ? rr_bytes / sizeof(pcppx_dns_rr) : 1);
	if (msg_bytes != 0)
		std::memset(got_msgs.data(), 0xA5, msg_bytes);
	if (rr_bytes != 0)
		std::memset(got_rrs.data(), 0xA5, rr_bytes);
	std::vector<uint64_t> got_totals(PCPPX_DNS_TOTALS, 0xA5A5A5A5A5A5A5A5ull);
	pcppx_batch b{};
	b.data = data.data();
	b.offsets = offsets.data();
	b.caplens = caplens.data();
	b.data_len = h[1];
	b.n = (uint32_t)n;
	b.linktype = 1;
	pcppx_records r{};
	if (summary)
		r.summary = reinterpret_cast<pcppx_summary*>(rec.data());
	else
		r.brief = reinterpret_cast<pcppx_brief*>(rec.data());
	r.layers = layers.data();
	pcppx_dns_spec s{};
	s.sections = (uint8_t)h[4];
	s.max_msgs = (uint32_t)h[5];
	pcppx_dns_out o{};
	o.msgs = got_msgs.data();
	o.rrs = got_rrs.data();
	o.names = has_names ? got_names.data() : nullptr;
	o.names_cap = h[8];
	o.disposition = has_disp ? got_disp.data() : nullptr;
	o.max_msgs = (uint32_t)h[6];
	o.max_rrs = (uint32_t)h[7];
	o.totals = got_totals.data();
	const int rc = pcppx_dns_reference(&b, &r, (uint8_t)ml, &s, &o);
	if (rc != PCPPX_OK)
	{
		std::fprintf(stderr, "%s: pcppx_dns_reference returned %d\n", path, rc);
		return 1;
	}
	const bool same = got_totals == want_totals &&
	                  (msg_bytes == 0 || std::memcmp(got_msgs.data(), want_msgs.data(), msg_bytes) == 0) &&
	                  (rr_bytes == 0 || std::memcmp(got_rrs.data(), want_rrs.data(), rr_bytes) == 0) &&
	                  got_names == want_names && got_disp == want_disp;
	if (!same)
		std::fprintf(stderr, "%s: the result differs from the expected one\n", path);
	return same ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv)
{
	int worst = argc > 1 ? 0 : 2;
	for (int k = 1; k < argc; ++k)
	{
		const int rc = run(argv[k]);
		std::printf("%s %s\n", argv[k], rc == 0 ? "ok" : "FAILED");
		worst = rc > worst ? rc : worst;
	}
	return worst;
}
