// tlsfp_ref_check — pcppx_tlsfp_reference on cases written by tests/test_tlsfp.py, for a sanitizer build (host compiler,
// no HIP): tlsfp_ref_check <file>...
// A .case file: 13 u64 words (n, data_len, max_layers, summary?, client, server, max_hellos, max_recs, text_cap, text?,
// disposition?, record bytes, text bytes), then the arrays: data, offsets, caplens, records, layers, and the expected
// records, text, disposition and totals (every buffer whole, fill included).
// A .md5 file: the 16-byte RFC 1321 digests of the texts of 0, 1, 2, ... bytes, text byte i = (7 i + 3) mod 256: the
// library's MD5 (pcppx_tlsfp.h) is run on the same texts.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pcppx.h"
#include "pcppx_tlsfp.h"

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

int run_md5(const char* path)
{
	FILE* f = std::fopen(path, "rb");
	if (f == nullptr)
		return 2;
	std::vector<uint8_t> want(16);
	int checked = 0;
	for (uint32_t len = 0; read(f, want.data(), 16); ++len, ++checked)
	{
		std::vector<uint8_t> text(len), copy(len, 0xA5);
		for (uint32_t i = 0; i < len; ++i)
			text[i] = (uint8_t)(7 * i + 3);
		uint32_t block[16], digest[4];
		pcppx::tlsfp::Md5Sink<1> sink(block, copy.data());
		for (uint32_t i = 0; i < len; ++i)
			sink.put(text[i]);
		sink.finish(digest);
		uint8_t got[16];
		for (int k = 0; k < 16; ++k)
			got[k] = (uint8_t)(digest[k >> 2] >> (8 * (k & 3)));
		if (std::memcmp(got, want.data(), 16) != 0 || copy != text)
		{
			std::fprintf(stderr, "%s: the digest of %u bytes differs\n", path, len);
			std::fclose(f);
			return 1;
		}
	}
	std::fclose(f);
	return checked > 0 ? 0 : 2;
}

int run(const char* path)
{
	FILE* f = std::fopen(path, "rb");
	if (f == nullptr)
		return 2;
	uint64_t h[13];
	if (!read(f, h, sizeof h))
		return 2;
	const uint64_t n = h[0], ml = h[2], rec_bytes = h[11], text_bytes = h[12];
	const bool summary = h[3] != 0, has_text = h[9] != 0, has_disp = h[10] != 0;
	std::vector<uint8_t> data, rec, want_recs, want_text, want_disp;
	std::vector<uint64_t> offsets, want_totals;
	std::vector<uint32_t> caplens;
	std::vector<pcppx_layer> layers;
	const size_t disp_n = has_disp ? n + 4 : 0;
	bool ok = load(f, data, h[1]) && load(f, offsets, n) && load(f, caplens, n) &&
	          load(f, rec, n * (summary ? sizeof(pcppx_summary) : sizeof(pcppx_brief))) && load(f, layers, n * ml) &&
	          load(f, want_recs, rec_bytes) && load(f, want_text, has_text ? text_bytes : 0) &&
	          load(f, want_disp, disp_n) && load(f, want_totals, PCPPX_TLSFP_TOTALS);
	std::fclose(f);
	if (!ok)
		return 2;
	// exact-size heap buffers: a byte read or written past any of them is the sanitizer's to report
	std::vector<uint8_t> got_text(has_text ? text_bytes : 0, 0xA5), got_disp(disp_n, 0xA5);
	// (one record where the case has room for none: a null out->recs is refused)
	std::vector<pcppx_tlsfp_rec> got_recs(rec_bytes != 0 ? rec_bytes / sizeof(pcppx_tlsfp_rec) : 1);
	if (rec_bytes != 0)
		std::memset(got_recs.data(), 0xA5, rec_bytes);
	std::vector<uint64_t> got_totals(PCPPX_TLSFP_TOTALS, 0xA5A5A5A5A5A5A5A5ull);
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
	pcppx_tlsfp_spec s{};
	s.client = (uint8_t)h[4];
	s.server = (uint8_t)h[5];
	s.max_hellos = (uint32_t)h[6];
	pcppx_tlsfps o{};
	o.recs = got_recs.data();
	o.text = has_text ? got_text.data() : nullptr;
	o.text_cap = h[8];
	o.disposition = has_disp ? got_disp.data() : nullptr;
	o.max_recs = (uint32_t)h[7];
	o.totals = got_totals.data();
	const int rc = pcppx_tlsfp_reference(&b, &r, (uint8_t)ml, &s, &o);
	if (rc != PCPPX_OK)
	{
		std::fprintf(stderr, "%s: pcppx_tlsfp_reference returned %d\n", path, rc);
		return 1;
	}
	const bool same = got_totals == want_totals &&
	                  (rec_bytes == 0 || std::memcmp(got_recs.data(), want_recs.data(), rec_bytes) == 0) &&
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
		const std::string path = argv[k];
		const bool md5 = path.size() > 4 && path.compare(path.size() - 4, 4, ".md5") == 0;
		const int rc = md5 ? run_md5(argv[k]) : run(argv[k]);
		std::printf("%s %s\n", argv[k], rc == 0 ? "ok" : "FAILED");
		worst = rc > worst ? rc : worst;
	}
	return worst;
}
