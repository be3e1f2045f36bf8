// pcppx_http.h — the http contract of include/pcppx.h as inline functions that pcppx_http.hip (device) and
// pcppx_http_ref.cpp (host, also built with a host compiler alone) both compile: the argument rules, the layer rule
// (rules 2-3), the first lines (rules 4-5), the field and the walk (rules 6-7), the names (rule 8), the content length
// (rule 9) and the text (rule 10), over a sink that either counts or emits.
// No reads happen here but through the layer pointer the caller hands in, whose bytes [0, L) lie inside an in-bounds
// packet.
#pragma once

#include <stdint.h>
#include <string.h>

#include "pcppx.h"
#include "pcppx_args.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PCPPX_HTTP_FN __host__ __device__ __forceinline__
#else
#define PCPPX_HTTP_FN inline
#endif

namespace pcppx
{
namespace http
{
constexpr uint32_t kProtoRequest = 6;  // pcpp::HTTPRequest; pcpp::HTTPResponse is 7
constexpr uint32_t kNoColon = 0xFFFFFFFFu;

// the argument rules pcppx_http_device and pcppx_http_reference share (include/pcppx.h)
inline bool valid_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_http_spec* s,
                       const pcppx_http_out* o)
{
	if (!valid_source(b, r, max_layers) || s == nullptr || o == nullptr || o->totals == nullptr || o->msgs == nullptr ||
	    o->fields == nullptr)
		return false;
	if (s->kinds == 0 || s->kinds > 3 || s->fields > PCPPX_HTTP_FIELDS_ALL || s->text > 3 ||
	    s->n_names > PCPPX_HTTP_MAX_NAMES)
		return false;
	for (uint32_t k = 0; k < PCPPX_HTTP_MAX_NAMES; ++k)
	{
		const uint32_t len = s->name_len[k];
		if (k >= s->n_names ? len != 0 : (len == 0 || len > PCPPX_HTTP_NAME_MAX))
			return false;
		for (uint32_t j = 0; j < len; ++j)
			if (s->names[k][j] >= 'A' && s->names[k][j] <= 'Z')
				return false;
		for (uint32_t q = 0; q < k && k < s->n_names; ++q)
			if (s->name_len[q] == len && memcmp(s->names[q], s->names[k], len) == 0)
				return false;
	}
	return true;
}

// What rules 2-3 find in an in-bounds packet: its disposition, and for MSG the layer's first byte (from the packet's
// first byte), its length L and its kind.
struct Layer
{
	uint32_t disp, off, L, kind;
};

// cap: the packet's caplen; lay: its ml layer entries; n_layers / flags: of its summary or brief. Reads no packet byte.
PCPPX_HTTP_FN Layer find_layer(uint32_t cap, const pcppx_layer* lay, uint32_t n_layers, uint32_t ml, uint32_t flags,
                               uint32_t kinds)
{
	Layer r{ PCPPX_HTTP_NONE, 0, 0, 0 };
	const uint32_t nl = n_layers < ml ? n_layers : ml;
	for (uint32_t k = 0; k < nl; ++k)
	{
		const pcppx_layer E = lay[k];
		const uint32_t kind = (uint32_t)E.proto - kProtoRequest;
		if (kind <= 1)
		{
			if (E.hdr_len <= E.data_len && (uint32_t)E.offset + E.data_len <= cap && ((kinds >> kind) & 1) != 0)
				r = Layer{ PCPPX_HTTP_MSG, E.offset, E.data_len, kind };
			return r;  // the first HTTP entry decides: one that is not followed leaves the packet NONE
		}
	}
	const bool l7 =
	    (flags & PCPPX_F_NEEDS_HOST_L7) != 0 && ((flags & PCPPX_F_L7_HTTP) != 0 || (flags & PCPPX_F_L7_KNOWN) == 0);
	if ((flags & (PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC | PCPPX_F_DEPTH_OVERFLOW)) != 0 ||
	    n_layers > ml || l7)
		r.disp = PCPPX_HTTP_HOST;
	return r;
}

// ---- the scans: unaligned dword loads with the zero-byte test, byte loads for the last (L - a) mod 4 bytes; every one
// reads bytes of [a, L) only. A byte at a time was measured 2.5 times slower (profiles/http_bench.json).
typedef uint32_t __attribute__((aligned(1), may_alias)) u32_any;
PCPPX_HTTP_FN uint32_t load32(const uint8_t* p)  // the four bytes at p, little-endian, whatever p's alignment
{
	return *reinterpret_cast<const u32_any*>(p);
}
PCPPX_HTTP_FN uint32_t zero_bytes(uint32_t v)
{
	return (v - 0x01010101u) & ~v & 0x80808080u;  // the lowest flagged byte is the first zero byte
}

// the first byte c in [a, L), else L
PCPPX_HTTP_FN uint32_t find_byte(const uint8_t* d, uint32_t a, uint32_t L, uint32_t c)
{
	uint32_t j = a;
	const uint32_t cc = c * 0x01010101u;
	for (; j + 4 <= L; j += 4)
	{
		const uint32_t m = zero_bytes(load32(d + j) ^ cc);
		if (m != 0)
			return j + ((uint32_t)__builtin_ctz(m) >> 3);
	}
	for (; j < L; ++j)
		if (d[j] == c)
			return j;
	return L;
}

// the first '\n' in [a, L), else L; nul: the first NUL byte before it, else the same value
PCPPX_HTTP_FN uint32_t find_nl(const uint8_t* d, uint32_t a, uint32_t L, uint32_t& nul)
{
	uint32_t j = a, z = L;
	for (; j + 4 <= L; j += 4)
	{
		const uint32_t w = load32(d + j);
		const uint32_t zl = zero_bytes(w ^ 0x0A0A0A0Au), z0 = zero_bytes(w);
		if (z == L && z0 != 0)
			z = j + ((uint32_t)__builtin_ctz(z0) >> 3);
		if (zl != 0)
		{
			const uint32_t e = j + ((uint32_t)__builtin_ctz(zl) >> 3);
			nul = z < e ? z : e;
			return e;
		}
	}
	for (; j < L; ++j)
	{
		const uint32_t v = d[j];
		if (v == '\n')
		{
			nul = z < j ? z : j;
			return j;
		}
		if (v == 0 && z == L)
			z = j;
	}
	nul = z;
	return L;
}

PCPPX_HTTP_FN uint32_t lower(uint32_t v)
{
	return v >= 'A' && v <= 'Z' ? v + 32 : v;
}

// "x.y" at p: HttpVersionStringToEnum (HttpLayer.cpp:160-164)
PCPPX_HTTP_FN uint32_t version_of(const uint8_t* p)
{
	if (p[1] != '.')
		return PCPPX_HTTP_VERSION_UNKNOWN;
	if (p[0] == '0' && p[2] == '9')
		return 0;
	if (p[0] == '1' && (p[2] == '0' || p[2] == '1'))
		return 1 + (p[2] - '0');
	return PCPPX_HTTP_VERSION_UNKNOWN;
}

// What the first line gives a message (rules 4-5).
struct FirstLine
{
	uint32_t len, a_off, a_len, status, method, version;
	bool complete;
};

// the bytes of a method name as one little-endian word
constexpr uint64_t word_of(const char* s, uint32_t k = 0)
{
	return s[k] == 0 ? 0 : ((uint64_t)(uint8_t)s[k] << (8 * k)) | word_of(s, k + 1);
}

// rule 4
PCPPX_HTTP_FN FirstLine request_line(const uint8_t* d, uint32_t L)
{
	FirstLine r{ L, 0, 0, 0, PCPPX_HTTP_METHOD_UNKNOWN, PCPPX_HTTP_VERSION_UNKNOWN, false };
	if (L < 4)
		return r;
	// the method: a known one has at most 7 bytes, so a space behind byte 7 is no different from none
	uint64_t w = 0;
	uint32_t sp = 0;
	const uint32_t lim = L < 8 ? L : 8;
	for (; sp < lim && d[sp] != ' '; ++sp)
		w |= (uint64_t)d[sp] << (8 * sp);
	if (sp == 0 || sp == lim)
		return r;
	r.method = w == word_of("GET")       ? 0u
	           : w == word_of("HEAD")    ? 1u
	           : w == word_of("POST")    ? 2u
	           : w == word_of("PUT")     ? 3u
	           : w == word_of("DELETE")  ? 4u
	           : w == word_of("TRACE")   ? 5u
	           : w == word_of("OPTIONS") ? 6u
	           : w == word_of("CONNECT") ? 7u
	           : w == word_of("PATCH")   ? 8u
	                                     : (uint32_t)PCPPX_HTTP_METHOD_UNKNOWN;
	if (r.method == PCPPX_HTTP_METHOD_UNKNOWN)
		return r;
	const uint32_t u = sp + 1;  // <= L
	// the first " HTTP/" in [u, L): the spaces one by one
	uint32_t v = u;
	for (;; ++v)
	{
		v = find_byte(d, v, L, ' ');
		if (v + 6 > L)
			return r;
		if (d[v + 1] == 'H' && d[v + 2] == 'T' && d[v + 3] == 'T' && d[v + 4] == 'P' && d[v + 5] == '/')
			break;
	}
	if (v + 9 > L)
		return r;
	r.version = version_of(d + v + 6);
	r.a_off = u;
	r.a_len = v - u;
	uint32_t nul;
	const uint32_t e = find_nl(d, v + 6, L, nul);
	r.complete = e < L;
	r.len = e < L ? e + 1 : L;
	return r;
}

// rule 5
PCPPX_HTTP_FN FirstLine response_line(const uint8_t* d, uint32_t L)
{
	FirstLine r{ L, 0, 0, 0, PCPPX_HTTP_METHOD_UNKNOWN, PCPPX_HTTP_VERSION_UNKNOWN, false };
	if (L >= 8 && d[0] == 'H' && d[1] == 'T' && d[2] == 'T' && d[3] == 'P' && d[4] == '/')
		r.version = version_of(d + 5);
	uint32_t nul;
	const uint32_t e0 = find_nl(d, 0, L, nul);
	r.complete = e0 < L;
	r.len = e0 < L ? e0 + 1 : L;
	if (r.version == PCPPX_HTTP_VERSION_UNKNOWN || L < 14)  // a message needs a byte at 13 and a '\n' behind it
		return r;
	const uint32_t c0 = (uint32_t)d[9] - '0', c1 = (uint32_t)d[10] - '0', c2 = (uint32_t)d[11] - '0';
	if (c0 > 9 || c1 > 9 || c2 > 9)
		return r;
	const uint32_t e = e0 >= 13 ? e0 : find_nl(d, 13, L, nul);  // the first '\n' in [13, L)
	if (e >= L)
		return r;
	const uint32_t end = e > 13 && d[e - 1] == '\r' ? e - 1 : e;
	if (end == 13)
		return r;
	r.status = 100 * c0 + 10 * c1 + c2;
	r.a_off = 13;
	r.a_len = end - 13;
	return r;
}

// rule 6: a header field as HeaderField's constructor leaves it
struct Field
{
	uint32_t off, size, name_len, value_off, value_len;
	bool end, has_value;
};

// colon: the first ':' at or behind an earlier field's start (L: none), or kNoColon before any search; searched again
// only once it lies before off, so that the walk's searches never cover a byte twice.
PCPPX_HTTP_FN Field read_field(const uint8_t* d, uint32_t L, uint32_t off, uint32_t& colon)
{
	Field f{ off, 0, 0, 0, 0, true, false };
	uint32_t nul;
	const uint32_t e = find_nl(d, off, L, nul);
	f.size = e < L ? e - off + 1 : nul - off;
	if (f.size == 0 || d[off] == '\r' || d[off] == '\n')
		return f;
	f.end = false;
	if (colon == kNoColon || colon < off)
		colon = find_byte(d, off, L, ':');
	const uint32_t c = colon;
	if (c >= L || (e < L && c >= e))
	{
		f.name_len = f.size;
		return f;
	}
	f.name_len = c - off;
	uint32_t vp = c + 1;
	while (vp < L && d[vp] == ' ')
		++vp;
	if (vp >= L)
		return f;
	f.has_value = true;
	f.value_off = vp;
	f.value_len = e >= L ? L - vp : e - vp - (d[e - 1] == '\r' ? 1u : 0u);
	return f;
}

// rule 8: k with names[k] equal to the lowered name, else PCPPX_HTTP_NO_NAME
PCPPX_HTTP_FN uint32_t name_id(const uint8_t* d, const Field& f, const pcppx_http_spec* s)
{
	for (uint32_t k = 0; k < s->n_names; ++k)
	{
		if (s->name_len[k] != f.name_len)
			continue;
		uint32_t j = 0;
		while (j < f.name_len && lower(d[f.off + j]) == (uint8_t)s->names[k][j])
			++j;
		if (j == f.name_len)
			return k;
	}
	return PCPPX_HTTP_NO_NAME;
}

PCPPX_HTTP_FN bool is_content_length(const uint8_t* d, const Field& f)
{
	constexpr uint64_t lo = word_of("content-"), hi = word_of("length");
	if (f.name_len != 14)
		return false;
	uint64_t a = 0, b = 0;
	for (uint32_t j = 0; j < 8; ++j)
		a |= (uint64_t)lower(d[f.off + j]) << (8 * j);
	for (uint32_t j = 0; j < 6; ++j)
		b |= (uint64_t)lower(d[f.off + 8 + j]) << (8 * j);
	return a == lo && b == hi;
}

// rule 9: atoi of the value cut at its first NUL; range: the magnitude does not fit an int
PCPPX_HTTP_FN int32_t content_length_of(const uint8_t* d, const Field& f, bool& range)
{
	uint32_t j = f.value_off;
	const uint32_t end = f.has_value ? f.value_off + f.value_len : j;
	while (j < end && (d[j] == ' ' || (d[j] >= '\t' && d[j] <= '\r')))
		++j;
	bool neg = false;
	if (j < end && (d[j] == '+' || d[j] == '-'))
		neg = d[j++] == '-';
	uint64_t v = 0;
	for (; j < end && (uint32_t)d[j] - '0' <= 9; ++j)
		v = v > 0x7FFFFFFFull ? v : v * 10 + (d[j] - '0');  // once above, it stays above
	range = v > 0x7FFFFFFFull;
	return range ? 0 : (neg ? -(int32_t)v : (int32_t)v);
}

// What the walk gives a message.
struct Walk
{
	FirstLine fl;
	uint32_t header_len, n_fields, n_rec, text_len, flags;
	int32_t content_length;
};

// One emitted field, as the sinks get it.
struct Rec
{
	uint32_t name_off, name_len, value_off, value_len, text_len, name_id, flags;
};

// d: the layer's L bytes. The message's text goes to s.text() range by range, in order; every emitted field goes to
// s.field() after its value's bytes went to s.text().
template <class Sink>
PCPPX_HTTP_FN Walk walk(const uint8_t* d, uint32_t L, uint32_t kind, const pcppx_http_spec* spec, Sink& s)
{
	Walk r{};
	r.fl = kind == PCPPX_HTTP_REQUEST ? request_line(d, L) : response_line(d, L);
	r.flags = r.fl.complete ? PCPPX_HTTP_FIRST_LINE_COMPLETE : 0;
	if ((spec->text & PCPPX_HTTP_TEXT_FIRST_LINE) != 0 && r.fl.a_len != 0)
	{
		s.text(d, r.fl.a_off, r.fl.a_len);
		r.text_len = r.fl.a_len;
	}
	uint32_t colon = kNoColon, seen = 0;
	Field f = read_field(d, L, r.fl.len, colon);  // linked always
	for (;;)
	{
		r.header_len = f.off + f.size;
		r.flags = (r.flags & ~(uint32_t)PCPPX_HTTP_HEADER_COMPLETE) |
		          (f.end || f.name_len == 0 ? PCPPX_HTTP_HEADER_COMPLETE : 0);
		if (f.end)
			break;
		++r.n_fields;
		if ((r.flags & PCPPX_HTTP_HAS_CONTENT_LENGTH) == 0 && is_content_length(d, f))
		{
			bool range;
			r.content_length = content_length_of(d, f, range);
			r.flags |= PCPPX_HTTP_HAS_CONTENT_LENGTH | (range ? PCPPX_HTTP_CONTENT_LENGTH_RANGE : 0);
		}
		if (spec->fields != PCPPX_HTTP_FIELDS_NONE)
		{
			const uint32_t id = name_id(d, f, spec);
			if (id != PCPPX_HTTP_NO_NAME || spec->fields == PCPPX_HTTP_FIELDS_ALL)
			{
				Rec x{ f.off, f.name_len, f.value_off, f.value_len, 0, id, f.has_value ? PCPPX_HTTP_HAS_VALUE : 0u };
				if (id != PCPPX_HTTP_NO_NAME)
				{
					if (((seen >> id) & 1) == 0)
						x.flags |= PCPPX_HTTP_FIRST;
					seen |= 1u << id;
					if ((spec->text & PCPPX_HTTP_TEXT_VALUES) != 0 && f.has_value)
					{
						s.text(d, f.value_off, f.value_len);
						x.text_len = f.value_len;
						r.text_len += f.value_len;
					}
				}
				s.field(x);
				++r.n_rec;
			}
		}
		if (f.off + f.size >= L)
			break;
		const Field next = read_field(d, L, f.off + f.size, colon);
		if (next.size == 0)
			break;
		f = next;
	}
	return r;
}

// the measuring sink
struct CountSink
{
	PCPPX_HTTP_FN void text(const uint8_t*, uint32_t, uint32_t) {}
	PCPPX_HTTP_FN void field(const Rec&) {}
};

// The emitting sink: a message's records from fields[0] on and its text from position pos of out (when set).
struct EmitSink
{
	pcppx_http_field* fields;
	uint8_t* out;  // or null
	uint64_t pos;  // of the next text byte
	uint32_t msg;  // the message's record number

	PCPPX_HTTP_FN void text(const uint8_t* d, uint32_t at, uint32_t len)
	{
		if (out != nullptr)
			for (uint32_t j = 0; j < len; ++j)
				out[pos + j] = d[at + j];
		pos += len;
	}
	PCPPX_HTTP_FN void field(const Rec& x)
	{
		pcppx_http_field o;  // built whole and stored once: the record is 8-byte aligned, so the copy is three 64-bit stores
		o.text_pos = pos - x.text_len;
		o.msg = msg;
		o.name_offset = (uint16_t)x.name_off;
		o.name_len = (uint16_t)x.name_len;
		o.value_offset = (uint16_t)x.value_off;
		o.value_len = (uint16_t)x.value_len;
		o.text_len = (uint16_t)x.text_len;
		o.name_id = (uint8_t)x.name_id;
		o.flags = (uint8_t)x.flags;
		*fields++ = o;
	}
};

// A message's 48-byte record.
PCPPX_HTTP_FN void put_msg(pcppx_http_msg* m, uint64_t first_field, uint64_t text_pos, uint32_t index, const Layer& l,
                           const Walk& w)
{
	pcppx_http_msg o;
	o.first_field = first_field;
	o.text_pos = text_pos;
	o.index = index;
	o.content_length = w.content_length;
	o.layer_offset = (uint16_t)l.off;
	o.layer_len = (uint16_t)l.L;
	o.header_len = (uint16_t)w.header_len;
	o.first_line_len = (uint16_t)w.fl.len;
	o.n_fields = (uint16_t)w.n_fields;
	o.n_rec = (uint16_t)w.n_rec;
	o.a_offset = (uint16_t)w.fl.a_off;
	o.a_len = (uint16_t)w.fl.a_len;
	o.status_code = (uint16_t)w.fl.status;
	o.text_len = (uint16_t)w.text_len;
	o.kind = (uint8_t)l.kind;
	o.method = (uint8_t)w.fl.method;
	o.version = (uint8_t)w.fl.version;
	o.flags = (uint8_t)w.flags;
	*m = o;
}
}  // namespace http
}  // namespace pcppx
