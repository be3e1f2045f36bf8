// pcppx_sip.h — the sip contract of include/pcppx.h as inline functions that pcppx_sip.hip (device) and
// pcppx_sip_ref.cpp (host, also built with a host compiler alone) both compile: the argument rules, the dispatch
// (rules 2-8), the first lines (rules 9-10), the walk (rules 11-13, over pcppx_http.h's field and scans), the SDP body
// (rule 13) and the records, over a sink that either counts or emits.
// No reads happen here but through the packet pointer the caller hands in, whose bytes [0, cap) are in bounds.
#pragma once

#include "pcppx_http.h"

#define PCPPX_SIP_FN PCPPX_HTTP_FN

namespace pcppx
{
namespace sip
{
using http::CountSink;
using http::EmitSink;
using http::Field;
using http::find_byte;
using http::find_nl;
using http::kNoColon;
using http::load32;
using http::lower;
using http::Rec;
using http::word_of;

constexpr uint32_t kProtoTcp = 4, kProtoUdp = 5, kProtoTrailer = 30;  // pcpp::TCP, UDP, PacketTrailer
constexpr uint32_t kCodeUnknown = 0;

// the argument rules pcppx_sip_device and pcppx_sip_reference share (include/pcppx.h): http's, plus the SDP records
inline bool valid_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_sip_spec* s,
                       const pcppx_sip_out* o)
{
	if (o == nullptr || o->sdps == nullptr || o->reserved != 0)
		return false;
	const pcppx_http_out h{ reinterpret_cast<pcppx_http_msg*>(o->msgs), o->fields, o->text, o->text_cap, o->disposition,
		                    o->max_msgs, o->max_fields, o->totals };
	return http::valid_args(b, r, max_layers, s, &h);
}

// ---- the first-line tests of rules 7 and 8 ----

// SipRequestFirstLine::parseMethod: 0..13, else PCPPX_SIP_METHOD_UNKNOWN. A known method has at most 9 bytes, so a
// space behind byte 9 is no different from none.
PCPPX_SIP_FN uint32_t method_of(const uint8_t* d, uint32_t L)
{
	if (L < 4)
		return PCPPX_SIP_METHOD_UNKNOWN;
	uint64_t w = 0;
	uint32_t sp = 0, b8 = 0;
	const uint32_t lim = L < 10 ? L : 10;
	for (; sp < lim && d[sp] != ' '; ++sp)
	{
		if (sp < 8)
			w |= (uint64_t)d[sp] << (8 * sp);
		else
			b8 = (b8 << 8) | d[sp];  // byte 8, then byte 9 (which no method has)
	}
	if (sp == 0 || sp == lim)
		return PCPPX_SIP_METHOD_UNKNOWN;
	if (sp > 8)
		return sp == 9 && w == word_of("SUBSCRIB") && b8 == 'E' ? 7u : (uint32_t)PCPPX_SIP_METHOD_UNKNOWN;
	return w == word_of("INVITE")     ? 0u
	       : w == word_of("ACK")      ? 1u
	       : w == word_of("BYE")      ? 2u
	       : w == word_of("CANCEL")   ? 3u
	       : w == word_of("REGISTER") ? 4u
	       : w == word_of("PRACK")    ? 5u
	       : w == word_of("OPTIONS")  ? 6u
	       : w == word_of("NOTIFY")   ? 8u
	       : w == word_of("PUBLISH")  ? 9u
	       : w == word_of("INFO")     ? 10u
	       : w == word_of("REFER")    ? 11u
	       : w == word_of("MESSAGE")  ? 12u
	       : w == word_of("UPDATE")   ? 13u
	                                  : (uint32_t)PCPPX_SIP_METHOD_UNKNOWN;
}

// len(method) + 1: m_UriOffset
PCPPX_SIP_FN uint32_t uri_offset(uint32_t method)
{
	// a nibble each, INVITE's the lowest: 7 4 4 7 9 6 8 10 7 8 5 6 8 7
	return (uint32_t)((0x786587A8697447ull >> (4 * method)) & 15);
}

// parseStatusCodePure over p[0..2]: the code when the switch accepts it, else kCodeUnknown. The chars are signed and
// the sum wraps modulo 2^16.
PCPPX_SIP_FN uint32_t code_of(const uint8_t* p)
{
	const int32_t c0 = (int8_t)p[0], c1 = (int8_t)p[1], c2 = (int8_t)p[2];
	const uint32_t code = (uint32_t)((c0 - 48) * 100 + (c1 - 48) * 10 + (c2 - 48)) & 0xFFFFu;
	switch (code)
	{
	case 100: case 180: case 181: case 182: case 183: case 199:
	case 200: case 202: case 204:
	case 300: case 301: case 302: case 305: case 380:
	case 400: case 401: case 402: case 403: case 404: case 405: case 406: case 407: case 408: case 409: case 410:
	case 411: case 412: case 413: case 414: case 415: case 416: case 417: case 420: case 421: case 422: case 423:
	case 424: case 425: case 428: case 429: case 430: case 433: case 436: case 437: case 438: case 439: case 440:
	case 469: case 470: case 480: case 481: case 482: case 483: case 484: case 485: case 486: case 487: case 488:
	case 489: case 491: case 493: case 494:
	case 500: case 501: case 502: case 503: case 504: case 505: case 513: case 555: case 580:
	case 600: case 603: case 604: case 606: case 607: case 608:
		return code;
	default:
		return kCodeUnknown;
	}
}

// getStatusCodeAsInt() of an accepted code: StatusCodeEnumToInt (SipLayer.cpp:687-692) lists 425, 423, 424 where the
// enum has Sip423, Sip424, Sip425
PCPPX_SIP_FN uint32_t code_as_int(uint32_t code)
{
	return code == 423 ? 425u : code == 424 ? 423u : code == 425 ? 424u : code;
}

// SipResponseFirstLine::parseStatusCode
PCPPX_SIP_FN uint32_t status_of(const uint8_t* d, uint32_t L)
{
	return L >= 12 && d[11] == ' ' ? code_of(d + 8) : kCodeUnknown;
}

// SipResponseFirstLine::parseVersion is not empty
PCPPX_SIP_FN bool has_version(const uint8_t* d, uint32_t L)
{
	return L >= 8 && load32(d) == (uint32_t)word_of("SIP/") && find_byte(d, 4, L, ' ') < L;
}

// SipLayer::detectSipMessageType over L >= 4 bytes: 0 a request key, 1 the response key, 2 none
PCPPX_SIP_FN uint32_t key_of(const uint8_t* d)
{
	switch (load32(d))
	{
	case (uint32_t)word_of("INVI"): case (uint32_t)word_of("ACK "): case (uint32_t)word_of("BYE "):
	case (uint32_t)word_of("CANC"): case (uint32_t)word_of("REGI"): case (uint32_t)word_of("PRAC"):
	case (uint32_t)word_of("OPTI"): case (uint32_t)word_of("SUBS"): case (uint32_t)word_of("NOTI"):
	case (uint32_t)word_of("PUBL"): case (uint32_t)word_of("INFO"): case (uint32_t)word_of("REFE"):
	case (uint32_t)word_of("MESS"): case (uint32_t)word_of("UPDA"):
		return 0;
	case (uint32_t)word_of("SIP/"):
		return 1;
	default:
		return 2;
	}
}

// SipRequestFirstLine::parseFirstLine behind a known method (rule 8)
PCPPX_SIP_FN bool heuristic_request(const uint8_t* d, uint32_t L, uint32_t method)
{
	const uint32_t s1 = uri_offset(method) - 1;
	const uint32_t s2 = find_byte(d, s1 + 1, L, ' ');
	if (s2 >= L || s2 == s1 + 1)
		return false;
	uint32_t e = s2 + 1;
	while (e < L && d[e] != '\r' && d[e] != '\n')
		++e;
	if (e - s2 - 1 < 7)
		return false;
	return d[s2 + 1] == 'S' && d[s2 + 2] == 'I' && d[s2 + 3] == 'P' && d[s2 + 4] == '/';
}

PCPPX_SIP_FN bool sip_port(uint32_t p)
{
	return p == 5060 || p == 5061;
}

// a port that gates a dissector of UdpLayer.cpp:122-165 (rule 5)
PCPPX_SIP_FN bool gated(uint32_t sp, uint32_t dp)
{
	const auto either = [](uint32_t p) {
		return p == 1812 || p == 1813 || p == 3799 || p == 2152 || p == 2123 || p == 546 || p == 547 || p == 123 ||
		       p == 13400 || p == 3496 || p == 30490 || p == 51820;
	};
	return either(sp) || either(dp) || dp == 0 || dp == 7 || dp == 9;
}

// What rules 2-8 find in an in-bounds packet: its disposition, and for MSG the layer's first byte (from the packet's
// first byte), its length L, its kind, its path and its carrier.
struct Layer
{
	uint32_t disp, off, L, kind, via, tcp;
};

// pkt: the packet's cap bytes; lay: its ml layer entries; n_layers / flags: of its summary or brief.
PCPPX_SIP_FN Layer find_layer(const uint8_t* pkt, uint32_t cap, const pcppx_layer* lay, uint32_t n_layers, uint32_t ml,
                              uint32_t flags, uint32_t kinds)
{
	Layer r{ PCPPX_SIP_NONE, 0, 0, 0, 0, 0 };
	// rule 2
	if ((flags & (PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC | PCPPX_F_DEPTH_OVERFLOW)) != 0 ||
	    n_layers > ml || ((flags & PCPPX_F_NEEDS_HOST_L7) != 0 && (flags & PCPPX_F_L7_KNOWN) == 0))
	{
		r.disp = PCPPX_SIP_HOST;
		return r;
	}
	// rule 3
	if ((flags & PCPPX_F_NEEDS_HOST_L7) == 0 || (flags & (PCPPX_F_L7_HTTP | PCPPX_F_L7_SSL | PCPPX_F_L7_DNS)) != 0)
		return r;
	// rule 4
	uint32_t k = n_layers;
	for (uint32_t j = 0; j < n_layers; ++j)
		if (lay[j].proto == kProtoTcp || lay[j].proto == kProtoUdp)
			k = j;
	if (k == n_layers || !(k + 1 == n_layers || (k + 2 == n_layers && lay[k + 1].proto == kProtoTrailer)))
		return r;
	const pcppx_layer E = lay[k];
	if (E.hdr_len < 8 || E.hdr_len >= E.data_len || (uint32_t)E.offset + E.data_len > cap)
		return r;
	const uint8_t* h = pkt + E.offset;
	const uint32_t sp = ((uint32_t)h[0] << 8) | h[1], dp = ((uint32_t)h[2] << 8) | h[3];
	const uint8_t* d = h + E.hdr_len;
	const uint32_t L = (uint32_t)E.data_len - E.hdr_len;
	r.off = (uint32_t)E.offset + E.hdr_len;
	r.L = L;
	r.tcp = E.proto == kProtoTcp ? 1 : 0;
	const bool port = sip_port(sp) || sip_port(dp);
	bool found = false;
	if (r.tcp != 0 ? port : (port && !((sp == 68 && dp == 67) || (sp == 67 && (dp == 68 || dp == 67))) && dp != 4789))
	{
		// rule 7
		if (method_of(d, L) != PCPPX_SIP_METHOD_UNKNOWN)
			found = true;
		else if (status_of(d, L) != kCodeUnknown && (r.tcp != 0 || has_version(d, L)))
		{
			found = true;
			r.kind = PCPPX_SIP_RESPONSE;
		}
	}
	else if (r.tcp == 0 && !((sp == 68 && dp == 67) || (sp == 67 && (dp == 68 || dp == 67))) && dp != 4789 && L >= 4)
	{
		// rules 5 and 8
		const uint32_t key = key_of(d);
		if (key == 2)
			return r;
		if (gated(sp, dp))
		{
			r.disp = PCPPX_SIP_HOST;
			return r;
		}
		r.via = PCPPX_SIP_VIA_HEURISTIC;
		if (key == 0)
		{
			const uint32_t m = method_of(d, L);
			found = m != PCPPX_SIP_METHOD_UNKNOWN && heuristic_request(d, L, m);
		}
		else if (L >= 12)
		{
			const uint32_t s = find_byte(d, 4, L, ' ');
			if (s < L)
			{
				if (s + 4 >= L)
				{
					r.disp = PCPPX_SIP_HOST;  // the reference reads d[s + 4]
					return r;
				}
				found = d[s + 4] == ' ' && code_of(d + s + 1) != kCodeUnknown;
				r.kind = PCPPX_SIP_RESPONSE;
			}
		}
	}
	if (found && ((kinds >> r.kind) & 1) != 0)
		r.disp = PCPPX_SIP_MSG;
	return r;
}

// What the first line gives a message (rules 9-10).
struct FirstLine
{
	uint32_t len, a_off, a_len, status, method;
	bool complete, version;
};

// rule 9. d[-1] is the carrier header's last byte.
PCPPX_SIP_FN FirstLine request_line(const uint8_t* d, uint32_t L)
{
	FirstLine r{ L, 0, 0, 0, method_of(d, L), false, false };
	const uint32_t u = uri_offset(r.method);  // the method is known: its space is at u - 1 < L
	// the first " SIP/" in [u, L): the spaces one by one
	uint32_t v = u, from = 0;
	for (;; ++v)
	{
		v = find_byte(d, v, L, ' ');
		if (v + 5 > L)
			break;
		if (d[v + 1] == 'S' && d[v + 2] == 'I' && d[v + 3] == 'P' && d[v + 4] == '/')
		{
			r.version = v + 7 <= L;
			break;
		}
	}
	if (r.version)
	{
		r.a_off = u;
		r.a_len = v - u;
		if (r.a_len == 0)
			r.a_off = 0;
		from = v + 1;
	}
	else if (d[-1] == '\n')
	{
		r.len = 0;
		r.complete = true;
		return r;
	}
	uint32_t nul;
	const uint32_t e = find_nl(d, from, L, nul);
	r.complete = e < L;
	r.len = e < L ? e + 1 : L;
	return r;
}

// rule 10
PCPPX_SIP_FN FirstLine response_line(const uint8_t* d, uint32_t L)
{
	FirstLine r{ L, 0, 0, 0, PCPPX_SIP_METHOD_UNKNOWN, false, has_version(d, L) };
	uint32_t nul;
	const uint32_t e = find_nl(d, 0, L, nul);
	r.complete = e < L;
	r.len = e < L ? e + 1 : L;
	r.status = r.version ? code_as_int(status_of(d, L)) : kCodeUnknown;
	if (r.status != kCodeUnknown)  // L >= 12 and d[0..3] == "SIP/", so r.len >= 5
	{
		uint32_t x = r.len - 2;
		if (d[x] != '\r')
			++x;
		if (x > 12)
		{
			r.a_off = 12;
			r.a_len = x - 12;
		}
	}
	return r;
}

PCPPX_SIP_FN bool name_is(const uint8_t* d, const Field& f, const char* name, uint32_t len)
{
	if (f.name_len != len)
		return false;
	for (uint32_t j = 0; j < len; ++j)
		if (lower(d[f.off + j]) != (uint8_t)name[j])
			return false;
	return true;
}

// the 15 bytes "application/sdp" somewhere in [a, a + n)
PCPPX_SIP_FN bool has_sdp_type(const uint8_t* d, uint32_t a, uint32_t n)
{
	constexpr uint64_t lo = word_of("applicat"), hi = word_of("ion/sdp");
	for (uint32_t j = a; j + 15 <= a + n; ++j)
	{
		if (d[j] != 'a')
			continue;
		uint64_t x = 0, y = 0;
		for (uint32_t q = 0; q < 8; ++q)
			x |= (uint64_t)d[j + q] << (8 * q);
		for (uint32_t q = 0; q < 7; ++q)
			y |= (uint64_t)d[j + 8 + q] << (8 * q);
		if (x == lo && y == hi)
			return true;
	}
	return false;
}

// What the walk gives a message.
struct Walk
{
	FirstLine fl;
	uint32_t header_len, n_fields, n_rec, text_len, flags;
	int32_t content_length;
};

// d: the layer's L bytes (and d[-1]). The message's text goes to s.text() range by range, in order; every emitted
// field goes to s.field() after its value's bytes went to s.text(). http's walk (rules 6-10 there) with the SIP first
// lines and the SDP test.
template <class Sink>
PCPPX_SIP_FN Walk walk(const uint8_t* d, const Layer& l, const pcppx_sip_spec* spec, Sink& s)
{
	const uint32_t L = l.L;
	Walk r{};
	r.fl = l.kind == PCPPX_SIP_REQUEST ? request_line(d, L) : response_line(d, L);
	r.flags = (r.fl.complete ? PCPPX_SIP_FIRST_LINE_COMPLETE : 0) | (r.fl.version ? PCPPX_SIP_VERSION_KNOWN : 0) |
	          (l.tcp != 0 ? PCPPX_SIP_CARRIER_TCP : 0);
	if ((spec->text & PCPPX_HTTP_TEXT_FIRST_LINE) != 0 && r.fl.a_len != 0)
	{
		s.text(d, r.fl.a_off, r.fl.a_len);
		r.text_len = r.fl.a_len;
	}
	uint32_t colon = kNoColon, seen = 0;
	bool type_seen = false, type_sdp = false;
	Field f = http::read_field(d, L, r.fl.len, colon);  // linked always
	for (;;)
	{
		r.header_len = f.off + f.size;
		r.flags = (r.flags & ~(uint32_t)PCPPX_SIP_HEADER_COMPLETE) |
		          (f.end || f.name_len == 0 ? PCPPX_SIP_HEADER_COMPLETE : 0);
		if (f.end)
			break;
		++r.n_fields;
		if ((r.flags & PCPPX_SIP_HAS_CONTENT_LENGTH) == 0 && http::is_content_length(d, f))
		{
			bool range;
			r.content_length = http::content_length_of(d, f, range);
			r.flags |= PCPPX_SIP_HAS_CONTENT_LENGTH | (range ? PCPPX_SIP_CONTENT_LENGTH_RANGE : 0);
		}
		if (!type_seen && name_is(d, f, "content-type", 12))
		{
			type_seen = true;
			type_sdp = f.has_value && has_sdp_type(d, f.value_off, f.value_len);
		}
		if (spec->fields != PCPPX_HTTP_FIELDS_NONE)
		{
			const uint32_t id = http::name_id(d, f, spec);
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
		const Field next = http::read_field(d, L, f.off + f.size, colon);
		if (next.size == 0)
			break;
		f = next;
	}
	if (L > r.header_len && r.content_length > 0 && type_sdp)  // rule 13
		r.flags |= PCPPX_SIP_HAS_SDP;
	return r;
}

// ---- the SDP body (rule 13) ----

PCPPX_SIP_FN bool is_space(uint32_t c)
{
	return c == ' ' || (c >= '\t' && c <= '\r');
}

// The tokens of [a, end) that rule 13 reads -- 0, 1, 3, 4 and 5 -- and how many there are. Named members, no
// array: an indexed one would live in scratch memory on the device.
struct Tokens
{
	uint32_t off0, len0, off1, len1, off3, len3, off4, len4, off5, len5, count;
};

PCPPX_SIP_FN Tokens split(const uint8_t* d, uint32_t a, uint32_t end)
{
	Tokens t{};
	uint32_t j = a;
	for (;;)
	{
		while (j < end && is_space(d[j]))
			++j;
		if (j >= end)
			break;
		const uint32_t b = j;
		while (j < end && !is_space(d[j]))
			++j;
		const uint32_t n = j - b;
		if (t.count == 0)
			t.off0 = b, t.len0 = n;
		else if (t.count == 1)
			t.off1 = b, t.len1 = n;
		else if (t.count == 3)
			t.off3 = b, t.len3 = n;
		else if (t.count == 4)
			t.off4 = b, t.len4 = n;
		else if (t.count == 5)
			t.off5 = b, t.len5 = n;
		++t.count;
	}
	return t;
}

PCPPX_SIP_FN bool token_is(const uint8_t* d, uint32_t off, uint32_t len, const char* text, uint32_t n)
{
	if (len != n)
		return false;
	for (uint32_t j = 0; j < n; ++j)
		if (d[off + j] != (uint8_t)text[j])
			return false;
	return true;
}

// inet_pton(AF_INET) over [a, a + n) cut at its first NUL; the address's four bytes as a little-endian word of the
// network-order bytes
PCPPX_SIP_FN bool ipv4_of(const uint8_t* d, uint32_t a, uint32_t n, uint32_t& addr)
{
	uint32_t octets = 0, cur = 0, out = 0;
	bool digit = false;
	for (uint32_t j = a; j < a + n && d[j] != 0; ++j)
	{
		const uint32_t c = d[j];
		if (c - '0' <= 9)
		{
			if (digit && cur == 0)
				return false;  // a leading zero
			cur = cur * 10 + (c - '0');
			if (cur > 255)
				return false;
			if (!digit)
			{
				if (++octets > 4)
					return false;
				digit = true;
			}
		}
		else if (c == '.' && digit)
		{
			if (octets == 4)
				return false;
			out |= cur << (8 * (octets - 1));
			cur = 0;
			digit = false;
		}
		else
			return false;
	}
	if (octets < 4 || !digit)
		return false;
	addr = out | (cur << 24);
	return true;
}

// (uint16_t)atoi over [a, a + n) cut at its first NUL, as strtol saturates
PCPPX_SIP_FN uint32_t port_of(const uint8_t* d, uint32_t a, uint32_t n)
{
	uint32_t j = a;
	const uint32_t end = a + n;
	bool neg = false;
	if (j < end && (d[j] == '+' || d[j] == '-'))
		neg = d[j++] == '-';
	uint64_t v = 0;
	bool sat = false;
	for (; j < end && (uint32_t)d[j] - '0' <= 9; ++j)
	{
		const uint32_t c = d[j] - '0';
		if (v > (0x7FFFFFFFFFFFFFFFull - c) / 10)
			sat = true;
		v = v * 10 + c;
	}
	if (sat || v > 0x7FFFFFFFFFFFFFFFull)
		return neg ? 0u : 0xFFFFu;  // LONG_MIN / LONG_MAX, cut
	return (uint32_t)(neg ? 0 - v : v) & 0xFFFFu;
}

struct Sdp
{
	uint32_t n_fields, owner, audio, video, flags;
};

// read_field of pcppx_http.h with '=' for ':' and no space skipped
PCPPX_SIP_FN Field sdp_field(const uint8_t* d, uint32_t L, uint32_t off, uint32_t& sep)
{
	Field f{ off, 0, 0, 0, 0, true, false };
	uint32_t nul;
	const uint32_t e = find_nl(d, off, L, nul);
	f.size = e < L ? e - off + 1 : nul - off;
	if (f.size == 0 || d[off] == '\r' || d[off] == '\n')
		return f;
	f.end = false;
	if (sep == kNoColon || sep < off)
		sep = find_byte(d, off, L, '=');
	const uint32_t c = sep;
	if (c >= L || (e < L && c >= e))
	{
		f.name_len = f.size;
		return f;
	}
	f.name_len = c - off;
	const uint32_t vp = c + 1;
	if (vp >= L)
		return f;
	f.has_value = true;
	f.value_off = vp;
	f.value_len = e >= L ? L - vp : e - vp - (d[e - 1] == '\r' ? 1u : 0u);
	return f;
}

// d: the body's L bytes
PCPPX_SIP_FN Sdp sdp_of(const uint8_t* d, uint32_t L)
{
	Sdp r{};
	uint32_t sep = kNoColon;
	bool owner_seen = false;
	Field f = sdp_field(d, L, 0, sep);
	for (;;)
	{
		if (f.end)
			break;
		++r.n_fields;
		if (f.name_len == 1)
		{
			const uint32_t c = lower(d[f.off]);
			const uint32_t end = f.value_off + (f.has_value ? f.value_len : 0);
			if (c == 'o' && !owner_seen)
			{
				owner_seen = true;
				const Tokens t = split(d, f.value_off, end);
				uint32_t addr = 0;
				if (t.count >= 6 && token_is(d, t.off3, t.len3, "IN", 2) && token_is(d, t.off4, t.len4, "IP4", 3) &&
				    ipv4_of(d, t.off5, t.len5, addr) && addr != 0)
				{
					r.owner = addr;
					r.flags |= PCPPX_SIP_SDP_HAS_OWNER;
				}
			}
			else if (c == 'm' && (r.flags & (PCPPX_SIP_SDP_HAS_AUDIO | PCPPX_SIP_SDP_HAS_VIDEO)) !=
			                         (PCPPX_SIP_SDP_HAS_AUDIO | PCPPX_SIP_SDP_HAS_VIDEO))
			{
				const Tokens t = split(d, f.value_off, end);
				if (t.count >= 2)
				{
					if ((r.flags & PCPPX_SIP_SDP_HAS_AUDIO) == 0 && token_is(d, t.off0, t.len0, "audio", 5))
					{
						r.audio = port_of(d, t.off1, t.len1);
						r.flags |= PCPPX_SIP_SDP_HAS_AUDIO;
					}
					else if ((r.flags & PCPPX_SIP_SDP_HAS_VIDEO) == 0 && token_is(d, t.off0, t.len0, "video", 5))
					{
						r.video = port_of(d, t.off1, t.len1);
						r.flags |= PCPPX_SIP_SDP_HAS_VIDEO;
					}
				}
			}
		}
		if (f.off + f.size >= L)
			break;
		const Field next = sdp_field(d, L, f.off + f.size, sep);
		if (next.size == 0)
			break;
		f = next;
	}
	return r;
}

// An SDP body's 32-byte record.
PCPPX_SIP_FN void put_sdp(pcppx_sip_sdp* p, uint32_t msg, uint32_t index, uint32_t off, uint32_t len, const Sdp& x)
{
	pcppx_sip_sdp o{};
	o.msg = msg;
	o.index = index;
	o.offset = (uint16_t)off;
	o.len = (uint16_t)len;
	o.n_fields = (uint16_t)x.n_fields;
	o.audio_port = (uint16_t)x.audio;
	o.video_port = (uint16_t)x.video;
	o.flags = (uint8_t)x.flags;
	o.owner_ipv4[0] = (uint8_t)x.owner;
	o.owner_ipv4[1] = (uint8_t)(x.owner >> 8);
	o.owner_ipv4[2] = (uint8_t)(x.owner >> 16);
	o.owner_ipv4[3] = (uint8_t)(x.owner >> 24);
	*p = o;
}

// A message's 48-byte record.
PCPPX_SIP_FN void put_msg(pcppx_sip_msg* m, uint64_t first_field, uint64_t text_pos, uint32_t index, const Layer& l,
                          const Walk& w)
{
	pcppx_sip_msg o;
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
	o.via = (uint8_t)l.via;
	o.flags = (uint8_t)w.flags;
	*m = o;
}
}  // namespace sip
}  // namespace pcppx
