// pcppx_ssl.h — the ssl contract of include/pcppx.h as inline functions that pcppx_ssl.hip (device) and
// pcppx_ssl_ref.cpp (host, also built with a host compiler alone) both compile: the argument rules, the chain rule
// (rule 2), the entry walk (rule 3), the handshake walk (rule 4) and the hello records (rules 5-7), over a sink that
// either counts or emits. The session id, the cipher count and the extension list are pcppx_tlsfp.h's, unchanged; the
// message walk is this file's own (tlsfp's lacks rule 4's case (b)).
// No reads happen here but through the packet pointer the caller hands in, whose bytes [0, caplen) it has found in
// bounds.
#pragma once

#include <stdint.h>

#include "pcppx.h"
#include "pcppx_args.h"
#include "pcppx_tlsfp.h"

#define PCPPX_SSL_FN PCPPX_TLSFP_FN

namespace pcppx
{
namespace ssl
{
using tlsfp::be16;
constexpr uint32_t kProtoSSL = 18, kProtoTCP = 4;  // pcpp::SSL, pcpp::TCP
constexpr uint32_t kCcs = 20, kAlert = 21, kHandshake = 22, kAppData = 23;

// the argument rules pcppx_ssl_device and pcppx_ssl_reference share (include/pcppx.h)
inline bool valid_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_ssl_spec* s,
                       const pcppx_ssl_out* o)
{
	if (!valid_source(b, r, max_layers) || s == nullptr || o == nullptr || o->totals == nullptr || o->msgs == nullptr ||
	    o->hellos == nullptr)
		return false;
	return s->kinds <= 3 && s->reserved[0] == 0 && s->reserved[1] == 0 && s->reserved[2] == 0;
}

// SSLLayer::isSSLPort (SSLLayer.h:488-510)
PCPPX_SSL_FN bool is_ssl_port(uint32_t p)
{
	return p == 443 || p == 261 || p == 448 || p == 465 || p == 563 || p == 614 || p == 636 || p == 989 || p == 990 ||
	       p == 992 || p == 993 || p == 994 || p == 995;
}

// rule 2: the chain was not recorded to its end
PCPPX_SSL_FN bool incomplete_chain(uint32_t flags, uint32_t n_layers, uint32_t ml)
{
	const bool l7 =
	    (flags & PCPPX_F_NEEDS_HOST_L7) != 0 && ((flags & PCPPX_F_L7_SSL) != 0 || (flags & PCPPX_F_L7_KNOWN) == 0);
	return (flags & (PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC | PCPPX_F_DEPTH_OVERFLOW)) != 0 ||
	       n_layers > ml || l7;
}

// rule 3's bounds: the entry is followed
PCPPX_SSL_FN bool followed(const pcppx_layer& E, uint32_t cap)
{
	return E.proto == kProtoSSL && E.data_len >= 5 && E.hdr_len >= 5 && E.hdr_len <= E.data_len &&
	       (uint32_t)E.offset + E.data_len <= cap;
}

// rule 4 (b): the types createHandshakeMessage's switch knows
PCPPX_SSL_FN bool known_type(uint32_t t)
{
	return t <= 20 && ((0x11F817u >> t) & 1) != 0;  // 0, 1, 2, 4, 11..16, 20
}

// One hello, as the sinks get it. Positions from the packet's first byte.
struct Hello
{
	uint32_t msg_off, name_off, name_len, version, header_version, cipher, n_ciphers, n_ext, kind, layer, sid, flags;
};

// rules 5-7. p: the hello message's first byte; D >= 4 bytes of it are readable; M <= D. at: p's position in the packet.
PCPPX_SSL_FN Hello read_hello(const uint8_t* p, uint32_t at, uint32_t D, uint32_t M, uint32_t kind, uint32_t layer)
{
	Hello h{ at, 0, 0, 0, 0, 0, 0, 0, kind, layer, 0, 0 };
	if (D > 39)
		h.sid = p[38] < D - 39 ? p[38] : D - 39;
	h.header_version = D < 6 ? 0 : be16(p + 4);
	h.version = h.header_version;
	const uint32_t cs = 39 + h.sid;
	tlsfp::Ext x;
	if (kind == PCPPX_SSL_CLIENT)
	{
		h.n_ciphers = cs + 2 > D ? 0 : be16(p + cs) / 2;
		for (tlsfp::ExtList l(p, D, M, cs + 2 + 2 * h.n_ciphers + 2); l.next(p, x);)
		{
			++h.n_ext;
			if (x.type != 0 || (h.flags & PCPPX_SSL_HAS_SNI) != 0)
				continue;
			h.flags |= PCPPX_SSL_HAS_SNI;  // the first one decides
			if (x.len >= 5)
			{
				const uint32_t want = be16(p + x.data + 3), room = x.len - 5;
				h.name_off = at + x.data + 5;
				h.name_len = want < room ? want : room;
				if (want > room)
					h.flags |= PCPPX_SSL_SNI_TRUNCATED;
			}
			else if (x.len != 0)
				h.flags |= PCPPX_SSL_SNI_MALFORMED;
		}
		if (h.name_len == 0)
			h.name_off = 0;
	}
	else
	{
		if (cs + 2 <= D)
		{
			h.cipher = be16(p + cs);
			h.flags |= PCPPX_SSL_HAS_CIPHER;
		}
		bool seen43 = false;
		for (tlsfp::ExtList l(p, D, M, cs + 3); l.next(p, x);)
		{
			++h.n_ext;
			if (x.type != 43 || seen43)
				continue;
			seen43 = true;  // the first one decides
			if (x.len == 2)
				h.version = be16(p + x.data);
			else if (x.len == 3 && p[x.data] == 2)
				h.version = be16(p + x.data + 1);
		}
	}
	return h;
}

// rule 4: the hellos of the handshake entry at [off, off + 5 + R) go to s.hello() in ascending message offset
template <class Sink>
PCPPX_SSL_FN void walk_handshake(const uint8_t* pk, uint32_t off, uint32_t R, uint32_t layer, uint32_t kinds, Sink& s)
{
	uint32_t todo = kinds;  // bit 0: the ClientHello is still to find; bit 1: the ServerHello
	for (uint32_t cur = 0; todo != 0 && R - cur >= 4;)  // M >= 4: at most R / 4 messages
	{
		const uint32_t D = R - cur, at = off + 5 + cur;
		const uint8_t* p = pk + at;
		if (D >= 16 && ((p[0] | p[1] | p[2] | p[3] | p[4]) == 0 || p[1] >= 1))
			break;  // (a): an unknown message takes the rest
		const uint32_t type = p[0];
		if (!known_type(type))
			break;  // (b)
		const uint32_t len = 4 + be16(p + 2), M = len < D ? len : D;
		if ((type == 1 || type == 2) && ((todo >> (type - 1)) & 1) != 0)
		{
			todo &= ~(1u << (type - 1));
			s.hello(pk, read_hello(p, at, D, M, type, layer));
		}
		cur += M;
	}
}

// What rules 2-4 give an in-bounds packet.
struct Pkt
{
	uint32_t disp, off0, payload_len, src_port, dst_port, ssl_port, flags;
	uint32_t n_type;  // the followed entries of type 20, 21, 22, 23: a byte each (at most PCPPX_MAX_LAYERS entries)
};

static_assert(PCPPX_MAX_LAYERS <= 255, "a byte per record type never overflows, so it never saturates either");
PCPPX_SSL_FN uint32_t type_count(const Pkt& w, uint32_t type)
{
	return (w.n_type >> (8 * (type - kCcs))) & 0xFFu;
}

// pk: the packet's cap bytes; lay: its ml layer entries; n_layers / flags: of its summary or brief.
template <class Sink>
PCPPX_SSL_FN Pkt walk(const uint8_t* pk, uint32_t cap, const pcppx_layer* lay, uint32_t n_layers, uint32_t ml,
                      uint32_t flags, uint32_t kinds, Sink& s)
{
	Pkt r{ PCPPX_SSL_NONE, 0, 0, 0, 0, 0, 0, 0 };
	if (incomplete_chain(flags, n_layers, ml))
	{
		r.disp = PCPPX_SSL_HOST;
		return r;
	}
	for (uint32_t k = 0; k < n_layers; ++k)  // n_layers <= ml here
	{
		const pcppx_layer E = lay[k];
		if (!followed(E, cap))
			continue;
		if (r.disp == PCPPX_SSL_NONE)
		{
			r.disp = PCPPX_SSL_MSG;
			r.off0 = E.offset;
			r.payload_len = E.data_len;
			r.flags = PCPPX_SSL_NO_TCP;
			if (k != 0)
			{
				const pcppx_layer T = lay[k - 1];
				if (T.proto == kProtoTCP && (uint32_t)T.offset + 4 <= cap)
				{
					r.flags = 0;
					r.src_port = be16(pk + T.offset);
					r.dst_port = be16(pk + T.offset + 2);
				}
			}
			r.ssl_port = is_ssl_port(r.src_port) ? r.src_port : r.dst_port;
		}
		const uint32_t type = pk[E.offset];
		if (type - kCcs <= 3)
			r.n_type += 1u << (8 * (type - kCcs));
		if (type == kHandshake)
			walk_handshake(pk, E.offset, (uint32_t)E.hdr_len - 5, k, kinds, s);
	}
	return r;
}

// the measuring sink
struct CountSink
{
	uint32_t n_hellos = 0, name_bytes = 0, n_client = 0;
	PCPPX_SSL_FN void hello(const uint8_t*, const Hello& h)
	{
		++n_hellos;
		name_bytes += h.name_len;
		n_client += h.kind == PCPPX_SSL_CLIENT ? 1u : 0u;
	}
};

// The emitting sink: a message's hello records from hellos[0] on and its names from position pos of names (when set).
struct EmitSink
{
	pcppx_ssl_hello* hellos;
	uint8_t* names;  // or null
	uint64_t pos;    // of the next name byte
	uint32_t msg;    // the message's record number
	uint32_t n_hellos = 0, name_bytes = 0;

	PCPPX_SSL_FN void hello(const uint8_t* pk, const Hello& h)
	{
		if (names != nullptr)
			for (uint32_t j = 0; j < h.name_len; ++j)
				names[pos + j] = pk[h.name_off + j];
		pcppx_ssl_hello o;  // built whole and stored once
		o.name_pos = pos;
		o.msg = msg;
		o.msg_offset = (uint16_t)h.msg_off;
		o.name_len = (uint16_t)h.name_len;
		o.version = (uint16_t)h.version;
		o.header_version = (uint16_t)h.header_version;
		o.cipher = (uint16_t)h.cipher;
		o.n_ciphers = (uint16_t)h.n_ciphers;
		o.n_ext = (uint16_t)h.n_ext;
		o.kind = (uint8_t)h.kind;
		o.layer = (uint8_t)h.layer;
		o.session_id_len = (uint8_t)h.sid;
		o.flags = (uint8_t)h.flags;
		o.reserved[0] = 0;
		o.reserved[1] = 0;
		*hellos++ = o;
		pos += h.name_len;
		name_bytes += h.name_len;
		++n_hellos;
	}
};

// A message's 32-byte record.
PCPPX_SSL_FN void put_msg(pcppx_ssl_msg* m, uint64_t first_hello, uint32_t index, const Pkt& w, uint32_t n_hellos,
                          uint32_t name_bytes)
{
	pcppx_ssl_msg o;
	o.first_hello = first_hello;
	o.index = index;
	o.name_bytes = name_bytes;
	o.layer_offset = (uint16_t)w.off0;
	o.payload_len = (uint16_t)w.payload_len;
	o.src_port = (uint16_t)w.src_port;
	o.dst_port = (uint16_t)w.dst_port;
	o.ssl_port = (uint16_t)w.ssl_port;
	o.n_handshake = (uint8_t)type_count(w, kHandshake);
	o.n_ccs = (uint8_t)type_count(w, kCcs);
	o.n_alert = (uint8_t)type_count(w, kAlert);
	o.n_appdata = (uint8_t)type_count(w, kAppData);
	o.n_hellos = (uint8_t)n_hellos;
	o.flags = (uint8_t)w.flags;
	*m = o;
}
}  // namespace ssl
}  // namespace pcppx
