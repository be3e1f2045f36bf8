// tcpstream_ref_check — pcppx_tcpstream_reference on cases written by tests/test_tcpstream.py, for a sanitizer build
// (host compiler, no HIP): tcpstream_ref_check <case file>...
// A case file: 12 u64 words (n, data_len, max_layers, summary?, base_clear, max_segments, max_streams, data_cap,
// index_only, columns?, streams bytes, data bytes), then the arrays: data, offsets, caplens, records, layers, info, and
// the expected streams, disposition, seg_stream, seg_pos, data and totals (every buffer whole, fill included).
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
	uint64_t h[12];
	if (!read(f, h, sizeof h))
		return 2;
	const uint64_t n = h[0], ml = h[2], streams_bytes = h[10], data_bytes = h[11];
	const bool summary = h[3] != 0, index_only = h[8] != 0, columns = h[9] != 0;
	std::vector<uint8_t> data, rec, want_streams, want_disp, want_data;
	std::vector<uint64_t> offsets, want_totals;
	std::vector<uint32_t> caplens, want_seg, want_pos;
	std::vector<pcppx_layer> layers;
	std::vector<pcppx_reasm_info> info;
	const size_t cols = columns ? n + 4 : 0;
	bool ok = load(f, data, h[1]) && load(f, offsets, n) && load(f, caplens, n) &&
	          load(f, rec, n * (summary ? sizeof(pcppx_summary) : sizeof(pcppx_brief))) && load(f, layers, n * ml) &&
	          load(f, info, n) && load(f, want_streams, streams_bytes) && load(f, want_disp, cols) &&
	          load(f, want_seg, cols) && load(f, want_pos, cols) && load(f, want_data, index_only ? 0 : data_bytes) &&
	          load(f, want_totals, PCPPX_TCPS_TOTALS);
	std::fclose(f);
	if (!ok)
		return 2;
	// exact-size heap buffers: a byte read or written past any of them is the sanitizer's to report
	std::vector<uint8_t> got_streams(streams_bytes, 0xA5), got_disp(cols, 0xA5), got_data(index_only ? 0 : data_bytes, 0xA5);
	std::vector<uint32_t> got_seg(cols, 0xA5A5A5A5u), got_pos(cols, 0xA5A5A5A5u);
	std::vector<uint64_t> got_totals(PCPPX_TCPS_TOTALS, 0xA5A5A5A5A5A5A5A5ull);
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
	pcppx_tcpstream_spec s{};
	s.base_clear = (uint8_t)h[4];
	s.max_segments = (uint32_t)h[5];
	pcppx_tcpstreams o{};
	o.data = index_only ? nullptr : got_data.data();
	o.data_cap = h[7];
	o.streams = reinterpret_cast<pcppx_tcpstream_rec*>(got_streams.data());
	o.disposition = columns ? got_disp.data() : nullptr;
	o.seg_stream = columns ? got_seg.data() : nullptr;
	o.seg_pos = columns ? got_pos.data() : nullptr;
	o.max_streams = (uint32_t)h[6];
	o.totals = got_totals.data();
	if (pcppx_tcpstream_reference(&b, &r, (uint8_t)ml, info.data(), &s, &o) != PCPPX_OK)
		return 3;
	ok = got_totals == want_totals && got_streams == want_streams && got_disp == want_disp && got_seg == want_seg &&
	     got_pos == want_pos && got_data == want_data;
	std::printf("%s: %llu streams, %llu bytes, %s\n", path, (unsigned long long)got_totals[PCPPX_TCPS_STREAMS],
	            (unsigned long long)got_totals[PCPPX_TCPS_BYTES], ok ? "equal" : "DIFFERENT");
	return ok ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv)
{
	int rc = argc > 1 ? 0 : 2;
	for (int k = 1; k < argc; ++k)
	{
		const int one = run(argv[k]);
		rc = rc != 0 ? rc : one;
	}
	return rc;
}
