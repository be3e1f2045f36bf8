// dhcp_ref_check — pcppx_dhcp_reference on cases written by tests/test_dhcp.py, for a sanitizer build (host compiler,
// no HIP): dhcp_ref_check <file>...
// A .case file: 9 u64 words (n, data_len, max_layers, summary?, out max_msgs, max_options, values_cap, values?,
// disposition?), the 72-byte spec, then the arrays: data, offsets, caplens, records, layers, and the expected messages
// (max_msgs), option records (max_options), values (values_cap bytes), disposition (n) and totals.
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
	uint64_t h[9];
	pcppx_dhcp_spec s;
	if (!read(f, h, sizeof h) || !read(f, &s, sizeof s))
		return 2;
	const uint64_t n = h[0], ml = h[2], max_msgs = h[4], max_options = h[5], values_cap = h[6];
	const bool summary = h[3] != 0, has_values = h[7] != 0, has_disp = h[8] != 0;
	const size_t msg_bytes = max_msgs * sizeof(pcppx_dhcp_msg), option_bytes = max_options * sizeof(pcppx_dhcp_option);
	std::vector<uint8_t> data, rec, want_msgs, want_options, want_values, want_disp;
	std::vector<uint64_t> offsets, want_totals;
	std::vector<uint32_t> caplens;
	std::vector<pcppx_layer> layers;
	bool ok = load(f, data, h[1]) && load(f, offsets, n) && load(f, caplens, n) &&
	          load(f, rec, n * (summary ? sizeof(pcppx_summary) : sizeof(pcppx_brief))) && load(f, layers, n * ml) &&
	          load(f, want_msgs, msg_bytes) && load(f, want_options, option_bytes) &&
	          load(f, want_values, has_values ? values_cap : 0) && load(f, want_disp, has_disp ? n : 0) &&
	          load(f, want_totals, PCPPX_DHCP_TOTALS);
	std::fclose(f);
	if (!ok)
		return 2;
	// exact-size heap buffers: a byte read or written past any of them is the sanitizer's to report
	std::vector<uint8_t> got_values(has_values ? values_cap : 0, 0xA5), got_disp(has_disp ? n : 0, 0xA5);
	// (one entry where the case has room for none: a null out->msgs or out->options is refused)
	std::vector<pcppx_dhcp_msg> got_msgs(max_msgs != 0 ? max_msgs : 1);
	std::vector<pcppx_dhcp_option> got_options(max_options != 0 ? max_options : 1);
	if (msg_bytes != 0)
		std::memset(got_msgs.data(), 0xA5, msg_bytes);
	if (option_bytes != 0)
		std::memset(got_options.data(), 0xA5, option_bytes);
	std::vector<uint64_t> got_totals(PCPPX_DHCP_TOTALS, 0xA5A5A5A5A5A5A5A5ull);
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
	pcppx_dhcp_out o{};
	o.msgs = got_msgs.data();
	o.options = got_options.data();
	o.values = has_values ? got_values.data() : nullptr;
	o.values_cap = values_cap;
	o.disposition = has_disp ? got_disp.data() : nullptr;
	o.max_msgs = (uint32_t)max_msgs;
	o.max_options = (uint32_t)max_options;
	o.totals = got_totals.data();
	const int rc = pcppx_dhcp_reference(&b, &r, (uint8_t)ml, &s, &o);
	if (rc != PCPPX_OK)
	{
		std::fprintf(stderr, "%s: pcppx_dhcp_reference returned %d\n", path, rc);
		return 1;
	}
	const bool same = got_totals == want_totals &&
	                  (msg_bytes == 0 || std::memcmp(got_msgs.data(), want_msgs.data(), msg_bytes) == 0) &&
	                  (option_bytes == 0 || std::memcmp(got_options.data(), want_options.data(), option_bytes) == 0) &&
	                  got_values == want_values && got_disp == want_disp;
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
