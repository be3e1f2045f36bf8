// pcppx_dhcp.h — the dhcp contract of include/pcppx.h as inline functions that pcppx_dhcp.hip (device) and
// pcppx_dhcp_ref.cpp (host, also built with a host compiler alone) both compile: the argument rules, the dispatch
// (rules 2-7), the two option walks (rules 8-9), the typed values (rule 11) and the records, over a sink that either
// counts or emits.
// No reads happen here but through the packet pointer the caller hands in, whose bytes [0, cap) are in bounds.
#pragma once

#include <stdint.h>

#include "pcppx.h"
#include "pcppx_args.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PCPPX_DHCP_FN __host__ __device__ __forceinline__
#else
#define PCPPX_DHCP_FN inline
#endif

namespace pcppx
{
namespace dhcp
{
constexpr uint32_t kProtoUdp = 5, kProtoTrailer = 30;  // pcpp::UDP, PacketTrailer
constexpr uint32_t kV4Header = 240, kV6Header = 4;     // sizeof(dhcp_header), sizeof(dhcpv6_header)
constexpr uint32_t kPad = 0, kEnd = 255;               // DHCPOPT_PAD, DHCPOPT_END
constexpr uint32_t kOptLease = 51, kOptMsgType = 53, kOptServerId = 54;

// the argument rules pcppx_dhcp_device and pcppx_dhcp_reference share (include/pcppx.h)
inline bool valid_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_dhcp_spec* s,
                       const pcppx_dhcp_out* o)
{
	if (!valid_source(b, r, max_layers) || s == nullptr || o == nullptr || o->totals == nullptr || o->msgs == nullptr ||
	    o->options == nullptr || o->reserved != 0)
		return false;
	if (s->families == 0 || s->families > 3 || s->options > PCPPX_DHCP_OPTIONS_ALL || s->values > 1 ||
	    s->n_codes6 > PCPPX_DHCP_MAX_CODES6)
		return false;
	for (uint32_t k = 0; k < PCPPX_DHCP_MAX_CODES6; ++k)
		if (k >= s->n_codes6 ? s->want6[k] != 0 : (k != 0 && s->want6[k] <= s->want6[k - 1]))
			return false;
	return true;
}

// What rules 2-7 find in an in-bounds packet: its disposition, and for MSG the layer's first byte (from the packet's
// first byte), its length L and its family (4 or 6).
struct Layer
{
	uint32_t disp, off, L, family;
};

PCPPX_DHCP_FN bool radius_or_gtp(uint32_t p)
{
	return p == 1812 || p == 1813 || p == 3799 || p == 2152 || p == 2123;
}

// pkt: the packet's cap bytes; lay: its ml layer entries; n_layers / flags: of its summary or brief.
PCPPX_DHCP_FN Layer find_layer(const uint8_t* pkt, uint32_t cap, const pcppx_layer* lay, uint32_t n_layers, uint32_t ml,
                               uint32_t flags, uint32_t families)
{
	Layer r{ PCPPX_DHCP_NONE, 0, 0, 0 };
	// rule 2
	if ((flags & (PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC | PCPPX_F_DEPTH_OVERFLOW)) != 0 ||
	    n_layers > ml || ((flags & PCPPX_F_NEEDS_HOST_L7) != 0 && (flags & PCPPX_F_L7_KNOWN) == 0))
	{
		r.disp = PCPPX_DHCP_HOST;
		return r;
	}
	// rule 3
	if ((flags & PCPPX_F_NEEDS_HOST_L7) == 0 || (flags & (PCPPX_F_L7_HTTP | PCPPX_F_L7_SSL | PCPPX_F_L7_DNS)) != 0)
		return r;
	// rule 4
	uint32_t k = n_layers;
	for (uint32_t j = 0; j < n_layers; ++j)
		if (lay[j].proto == kProtoUdp)
			k = j;
	if (k == n_layers || !(k + 1 == n_layers || (k + 2 == n_layers && lay[k + 1].proto == kProtoTrailer)))
		return r;
	const pcppx_layer E = lay[k];
	if (E.hdr_len != 8 || E.data_len <= 8 || (uint32_t)E.offset + E.data_len > cap)
		return r;
	const uint8_t* h = pkt + E.offset;
	const uint32_t sp = ((uint32_t)h[0] << 8) | h[1], dp = ((uint32_t)h[2] << 8) | h[3];
	const uint32_t L = (uint32_t)E.data_len - 8;
	r.off = (uint32_t)E.offset + 8;
	r.L = L;
	if ((sp == 68 && dp == 67) || (sp == 67 && (dp == 68 || dp == 67)))
	{
		// rule 5
		if (L < kV4Header)
			return r;
		r.family = 4;
	}
	else
	{
		// rule 6
		const bool s6 = sp == 546 || sp == 547, d6 = dp == 546 || dp == 547;
		if (!s6 && !d6)
			return r;
		if (dp == 4789 || sp == 5060 || sp == 5061 || dp == 5060 || dp == 5061)
			return r;
		if (radius_or_gtp(sp) || radius_or_gtp(dp))  // a DHCPv6 port is none of them: this is the other port
		{
			r.disp = PCPPX_DHCP_HOST;
			return r;
		}
		if (L < kV6Header)
			return r;
		r.family = 6;
	}
	// rule 7
	if ((families & (r.family == 4 ? PCPPX_DHCP_V4 : PCPPX_DHCP_V6)) != 0)
		r.disp = PCPPX_DHCP_MSG;
	return r;
}

PCPPX_DHCP_FN uint32_t be16(const uint8_t* p)
{
	return ((uint32_t)p[0] << 8) | p[1];
}

PCPPX_DHCP_FN uint32_t be32(const uint8_t* p)
{
	return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// the four bytes at p as a little-endian word of the network-order bytes
PCPPX_DHCP_FN uint32_t le32(const uint8_t* p)
{
	return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// rule 10: whether an option of this code gets a record
PCPPX_DHCP_FN bool wanted(const pcppx_dhcp_spec* spec, uint32_t family, uint32_t code)
{
	if (spec->options != PCPPX_DHCP_OPTIONS_WANTED)
		return spec->options == PCPPX_DHCP_OPTIONS_ALL;
	if (family == 4)
		return ((spec->want4[code >> 5] >> (code & 31)) & 1) != 0;
	for (uint32_t k = 0; k < spec->n_codes6; ++k)
		if (spec->want6[k] == code)
			return true;
	return false;
}

// What the walk gives a message. server_id: le32 of the four bytes.
struct Walk
{
	uint32_t n_options, options_len, n_rec, value_len, msg_type, lease_time, server_id, flags;
};

// d: the layer's L bytes. Every emitted option goes to s.option() with the position of its value among the message's
// emitted value bytes.
template <class Sink>
PCPPX_DHCP_FN Walk walk(const uint8_t* d, uint32_t L, uint32_t family, const pcppx_dhcp_spec* spec, Sink& s)
{
	Walk r{};
	const bool v4 = family == 4;
	uint32_t p = v4 ? kV4Header : kV6Header;
	const uint32_t first = p;
	bool seen_type = false, seen_lease = false, seen_server = false;
	for (;;)
	{
		const uint32_t rem = L - p;  // p <= L throughout
		uint32_t code, len, head;
		if (v4)
		{
			// rule 8
			if (rem < 1)
				break;
			code = d[p];
			if (code == kPad || code == kEnd)
			{
				len = 0;
				head = 1;
			}
			else
			{
				if (rem < 2)
					break;
				len = d[p + 1];
				head = 2;
			}
		}
		else
		{
			// rule 9
			if (rem < 4)
				break;
			code = be16(d + p);
			len = be16(d + p + 2);
			head = 4;
		}
		if (head + len > rem)
			break;
		const uint32_t v = p + head;  // the value's first byte
		if (v4)
		{
			// rule 11: the first option of each code
			if (code == kOptMsgType && !seen_type)
			{
				seen_type = true;
				r.flags |= PCPPX_DHCP_HAS_MSG_TYPE;
				r.msg_type = len >= 1 ? d[v] : 0u;
			}
			else if (code == kOptLease && !seen_lease)
			{
				seen_lease = true;
				if (len >= 4)
				{
					r.lease_time = be32(d + v);
					r.flags |= PCPPX_DHCP_HAS_LEASE_TIME;
				}
			}
			else if (code == kOptServerId && !seen_server)
			{
				seen_server = true;
				if (len >= 4)
				{
					r.server_id = le32(d + v);
					r.flags |= PCPPX_DHCP_HAS_SERVER_ID;
				}
			}
		}
		if (wanted(spec, family, code))
		{
			const uint32_t copied = spec->values != 0 ? len : 0u;
			s.option(d, code, len, p, r.n_options, v, r.value_len, copied);
			++r.n_rec;
			r.value_len += copied;
		}
		++r.n_options;
		p = v + len;
	}
	r.options_len = p - first;
	return r;
}

// PCPPX_DHCP_REPLY of a message: the BOOTP op of a DHCPv4 header
PCPPX_DHCP_FN bool is_reply(const uint8_t* d, uint32_t family)
{
	return family == 4 && d[0] == 2;
}

// the measuring sink
struct CountSink
{
	PCPPX_DHCP_FN void option(const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}
};

// The emitting sink: a message's records from options[0] on and its value bytes from position pos of out (when set).
struct EmitSink
{
	pcppx_dhcp_option* options;
	uint8_t* out;  // or null
	uint64_t pos;  // of the message's first value byte
	uint32_t msg;  // the message's record number

	PCPPX_DHCP_FN void option(const uint8_t* d, uint32_t code, uint32_t len, uint32_t off, uint32_t ordinal,
	                          uint32_t value_at, uint32_t value_rel, uint32_t copied)
	{
		if (out != nullptr)
			for (uint32_t j = 0; j < copied; ++j)
				out[pos + value_rel + j] = d[value_at + j];
		pcppx_dhcp_option o;  // built whole and stored once: the record is 4-byte aligned
		o.msg = msg;
		o.code = (uint16_t)code;
		o.len = (uint16_t)len;
		o.offset = (uint16_t)off;
		o.ordinal = (uint16_t)ordinal;
		o.value_rel = (uint16_t)value_rel;
		o.reserved = 0;
		*options++ = o;
	}
};

// A message's 80-byte record. d: the layer's bytes (L >= 240 for family 4, >= 4 for family 6).
PCPPX_DHCP_FN void put_msg(pcppx_dhcp_msg* m, uint64_t first_option, uint64_t value_pos, uint32_t index,
                           const uint8_t* d, const Layer& l, const Walk& w)
{
	pcppx_dhcp_msg o{};
	o.first_option = first_option;
	o.value_pos = value_pos;
	o.index = index;
	o.lease_time = w.lease_time;
	o.layer_offset = (uint16_t)l.off;
	o.layer_len = (uint16_t)l.L;
	o.n_options = (uint16_t)w.n_options;
	o.n_rec = (uint16_t)w.n_rec;
	o.value_len = (uint16_t)w.value_len;
	o.options_len = (uint16_t)w.options_len;
	o.family = (uint8_t)l.family;
	uint32_t flags = w.flags;
	if (l.family == 4)
	{
		o.op = d[0];
		o.htype = d[1];
		o.hlen = d[2];
		o.hops = d[3];
		o.xid = be32(d + 4);
		o.secs = (uint16_t)be16(d + 8);
		o.bootp_flags = (uint16_t)be16(d + 10);
		for (uint32_t j = 0; j < 4; ++j)
		{
			o.ciaddr[j] = d[12 + j];
			o.yiaddr[j] = d[16 + j];
			o.siaddr[j] = d[20 + j];
			o.giaddr[j] = d[24 + j];
			o.server_id[j] = (uint8_t)(w.server_id >> (8 * j));
		}
		if (o.htype == 1 && o.hlen == 6)
		{
			flags |= PCPPX_DHCP_HAS_MAC;
			for (uint32_t j = 0; j < 6; ++j)
				o.client_mac[j] = d[28 + j];
		}
		if (be32(d + 236) == 0x63825363u)
			flags |= PCPPX_DHCP_MAGIC_OK;
		if (o.op == 2)
			flags |= PCPPX_DHCP_REPLY;
		o.msg_type = (uint8_t)w.msg_type;
	}
	else
	{
		o.msg_type = d[0] <= 13 ? d[0] : (uint8_t)0;
		o.xid = ((uint32_t)d[1] << 16) | ((uint32_t)d[2] << 8) | d[3];
	}
	o.flags = (uint8_t)flags;
	*m = o;
}
}  // namespace dhcp
}  // namespace pcppx
