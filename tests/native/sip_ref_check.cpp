// sip_ref_check — pcppx_sip_reference on cases written by tests/test_sip.py, for a sanitizer build (host compiler,
// no HIP): sip_ref_check <file>...
// A .case file: 10 u64 words (n, data_len, max_layers, summary?, out max_msgs, max_fields, max_sdps, text_cap, text?,
// disposition?), the 272-byte spec, then the arrays: data, offsets, caplens, records, layers, and the expected messages
// (max_msgs), field records (max_fields), SDP records (max_sdps), text (text_cap bytes), disposition (n) and totals.
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
	uint64_t h[10];
	pcppx_sip_spec s;
	if (!read(f, h, sizeof h) || !read(f, &s, sizeof s))
		return 2;
	const uint64_t n = h[0], ml = h[2], max_msgs = h[4], max_fields = h[5], max_sdps = h[6], text_cap = h[7];
	const bool summary = h[3] != 0, has_text = h[8] != 0, has_disp = h[9] != 0;
	const size_t msg_bytes = max_msgs * sizeof(pcppx_sip_msg), field_bytes = max_fields * sizeof(pcppx_sip_field),
	             sdp_bytes = max_sdps * sizeof(pcppx_sip_sdp);
	std::vector<uint8_t> data, rec, want_msgs, want_fields, want_sdps, want_text, want_disp;
	std::vector<uint64_t> offsets, want_totals;
	std::vector<uint32_t> caplens;
	std::vector<pcppx_layer> layers;
	bool ok = load(f, data, h[1]) && load(f, offsets, n) && load(f, caplens, n) &&
	          load(f, rec, n * (summary ? sizeof(pcppx_summary) : sizeof(pcppx_brief))) && load(f, layers, n * ml) &&
	          load(f, want_msgs, msg_bytes) && load(f, want_fields, field_bytes) && load(f, want_sdps, sdp_bytes) &&
	          load(f, want_text, has_text ? text_cap : 0) && load(f, want_disp, has_disp ? n : 0) &&
	          load(f, want_totals, PCPPX_SIP_TOTALS);
	std::fclose(f);
	if (!ok)
		return 2;
	// exact-size heap buffers: a byte read or written past any of them is the sanitizer's to report. The data is exact
	// too, so the one byte rule 9 reads in front of a layer is inside it or reported.
	std::vector<uint8_t> got_text(has_text ? text_cap : 0, 0xA5), got_disp(has_disp ? n : 0, 0xA5);
	// (one entry where the case has room for none: a null out->msgs, out->fields or out->sdps is refused)
	std::vector<pcppx_sip_msg> got_msgs(max_msgs != 0 ? max_msgs : 1);
	std::vector<pcppx_sip_field> got_fields(max_fields != 0 ? max_fields : 1);
	std::vector<pcppx_sip_sdp> got_sdps(max_sdps != 0 ? max_sdps : 1);
	if (msg_bytes != 0)
		std::memset(got_msgs.data(), 0xA5, msg_bytes);
	if (field_bytes != 0)
		std::memset(got_fields.data(), 0xA5, field_bytes);
	if (sdp_bytes != 0)
		std::memset(got_sdps.data(), 0xA5, sdp_bytes);
	std::vector<uint64_t> got_totals(PCPPX_SIP_TOTALS, 0xA5A5A5A5A5A5A5A5ull);
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
	pcppx_sip_out o{};
	o.msgs = got_msgs.data();
	o.fields = got_fields.data();
	o.sdps = got_sdps.data();
	o.text = has_text ? got_text.data() : nullptr;
	o.text_cap = text_cap;
	o.disposition = has_disp ? got_disp.data() : nullptr;
	o.max_msgs = (uint32_t)max_msgs;
	o.max_fields = (uint32_t)max_fields;
	o.max_sdps = (uint32_t)max_sdps;
	o.totals = got_totals.data();
	const int rc = pcppx_sip_reference(&b, &r, (uint8_t)ml, &s, &o);
	if (rc != PCPPX_OK)
	{
		std::fprintf(stderr, "%s: pcppx_sip_reference returned %d\n", path, rc);
		return 1;
	}
	const bool same = got_totals == want_totals &&
	                  (msg_bytes == 0 || std::memcmp(got_msgs.data(), want_msgs.data(), msg_bytes) == 0) &&
	                  (field_bytes == 0 || std::memcmp(got_fields.data(), want_fields.data(), field_bytes) == 0) &&
	                  (sdp_bytes == 0 || std::memcmp(got_sdps.data(), want_sdps.data(), sdp_bytes) == 0) &&
	                  got_text == want_text && got_disp == want_disp;
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
