// pcppx_dns.h — the dns contract of include/pcppx.h as inline functions that pcppx_dns.hip (device) and
// pcppx_dns_ref.cpp (host, also built with a host compiler alone) both compile: the argument rules, the layer rule
// (rules 2-3), the resource walk (rule 4) and the name decode (rule 5), over a sink that either counts or emits.
// No reads happen here but through the layer pointer the caller hands in, whose bytes [0, L) lie inside an in-bounds
// packet.
#pragma once

#include <stdint.h>

#include "pcppx.h"
#include "pcppx_args.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PCPPX_DNS_FN __host__ __device__ __forceinline__
#else
#define PCPPX_DNS_FN inline
#endif

namespace pcppx
{
namespace dns
{
constexpr uint32_t kProtoDNS = 13;      // pcpp::DNS
constexpr uint32_t kProtoTCP = 4;       // pcpp::TCP
constexpr uint32_t kHeader = 12;        // sizeof(dnshdr)
constexpr uint32_t kMaxResources = 300; // DnsLayer.cpp:145
constexpr uint32_t kMaxLevel = 20;      // DnsResource.cpp:62; a resource's own name is level 1 (DnsResource.h:43)

// the argument rules pcppx_dns_device and pcppx_dns_reference share (include/pcppx.h)
inline bool valid_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_dns_spec* s,
                       const pcppx_dns_out* o)
{
	if (!valid_source(b, r, max_layers) || s == nullptr || o == nullptr || o->totals == nullptr || o->msgs == nullptr ||
	    o->rrs == nullptr)
		return false;
	if (s->sections == 0 || s->sections > 15)
		return false;
	return s->reserved[0] == 0 && s->reserved[1] == 0 && s->reserved[2] == 0;
}

PCPPX_DNS_FN uint32_t be16(const uint8_t* p)
{
	return ((uint32_t)p[0] << 8) | p[1];
}

// What rules 2-3 find in an in-bounds packet: its disposition, and for MSG the layer's first byte (from the packet's
// first byte), its length L and the TCP adjustment.
struct Layer
{
	uint32_t disp, off, L, adj;
};

// cap: the packet's caplen; lay: its ml layer entries; n_layers / flags: of its summary or brief. Reads no packet byte.
PCPPX_DNS_FN Layer find_layer(uint32_t cap, const pcppx_layer* lay, uint32_t n_layers, uint32_t ml, uint32_t flags)
{
	Layer r{ PCPPX_DNS_NONE, 0, 0, 0 };
	const uint32_t nl = n_layers < ml ? n_layers : ml;
	uint32_t prev = 0xFFFFFFFFu;
	for (uint32_t k = 0; k < nl; ++k)
	{
		const pcppx_layer E = lay[k];
		if (E.proto == kProtoDNS)
		{
			const uint32_t adj = prev == kProtoTCP ? 2u : 0u;
			if (E.hdr_len <= E.data_len && (uint32_t)E.offset + E.data_len <= cap && E.data_len >= kHeader + adj)
				r = Layer{ PCPPX_DNS_MSG, E.offset, E.data_len, adj };
			return r;  // the first DNS entry decides: one that is not followed leaves the packet NONE
		}
		prev = E.proto;
	}
	const bool l7 =
	    (flags & PCPPX_F_NEEDS_HOST_L7) != 0 && ((flags & PCPPX_F_L7_DNS) != 0 || (flags & PCPPX_F_L7_KNOWN) == 0);
	if ((flags & (PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC | PCPPX_F_DEPTH_OVERFLOW)) != 0 ||
	    n_layers > ml || l7)
		r.disp = PCPPX_DNS_HOST;
	return r;
}

// ---- rule 5: IDnsResource::decodeName without its recursion ----
// A level is a run of labels; after a pointer a level only returns, so the levels form a chain. The first level (the
// reference's iteration 1) alone decides the encoded length and whether the name fails; name_scan walks it by label
// lengths without touching the text.
struct NameScan
{
	uint32_t name_len;
	bool ok;
};

// d: the layer's L bytes; off: where the name starts (any value).
PCPPX_DNS_FN NameScan name_scan(const uint8_t* d, uint32_t L, uint32_t off, uint32_t adj)
{
	if (off + 1 > L)
		return { 0, true };
	uint32_t enc = 0, cur = off;
	for (;;)  // enc grows by at least 2 a turn and stops the loop above 255
	{
		const uint32_t w = d[cur];
		if (w == 0)
			return { enc + (enc < 256 ? 1u : 0u), true };
		if ((w & 0xC0) == 0xC0)
		{
			if (cur + 2 > L || enc > 255)
				return { enc + (enc < 256 ? 1u : 0u), true };
			const uint32_t to = ((((w & 0x3F) << 8) | d[cur + 1]) + adj) & 0xFFFF;
			if (to < kHeader || to >= L)
				return { 0, false };
			return { enc + 2, true };
		}
		if (cur + w + 1 > L || enc + w > 255)
			return { enc == 256 ? 256u : enc + 1, true };
		cur += w + 1;
		enc += w + 1;
		if (cur + 1 > L)
			return { enc == 256 ? 256u : enc + 1, true };
	}
}

// The text of a name whose name_scan gave ok and name_len > 0, every byte through s.put() in order; returns its
// length. One running budget stands for the nested "at most 255 decoded bytes per level" limits: a level's tail may
// take what the levels above leave and 255 minus the level's own encoded bytes. The one byte a level may take back (the
// dot cleanup() strips, or the one the 256-byte cut drops) is held back until the next byte or the end decides; a NUL
// byte inside a label ends the text (the callers copy C strings).
template <class Sink>
PCPPX_DNS_FN uint32_t name_text(const uint8_t* d, uint32_t L, uint32_t off, uint32_t adj, Sink& s)
{
	uint32_t budget = 512, len = 0, cur = off, held = 0;
	bool have = false, last_out = false, strip = false;
	auto out = [&](uint32_t v) {
		if (budget == 0 || v == 0)
		{
			budget = 0;
			last_out = false;
			return;
		}
		if (have)
		{
			s.put((uint8_t)held);
			++len;
		}
		held = v;
		have = true;
		last_out = true;
		--budget;
	};
	for (uint32_t level = 1; level <= kMaxLevel && cur + 1 <= L; ++level)
	{
		uint32_t enc = 0;
		bool jump = false;
		last_out = false;
		for (;;)
		{
			const uint32_t w = d[cur];
			if (w == 0)
			{
				strip = enc != 0;
				break;
			}
			if ((w & 0xC0) == 0xC0)
			{
				if (cur + 2 > L || enc > 255)
				{
					strip = enc != 0;
					break;
				}
				const uint32_t to = ((((w & 0x3F) << 8) | d[cur + 1]) + adj) & 0xFFFF;
				if (to < kHeader || to >= L)
					break;  // a nested level fails: its labels so far stay, dot included
				budget = budget < 255 - enc ? budget : 255 - enc;
				cur = to;
				jump = budget != 0;  // with nothing left no later level can add or take back a byte
				break;
			}
			if (cur + w + 1 > L || enc + w > 255)
			{
				strip = enc == 256;
				break;
			}
			for (uint32_t j = 1; j <= w; ++j)
				out(d[cur + j]);
			out('.');
			cur += w + 1;
			enc += w + 1;
			if (cur + 1 > L)
			{
				strip = enc == 256;
				break;
			}
		}
		if (!jump)
			break;
		strip = false;
	}
	if (have && !(strip && last_out))
	{
		s.put((uint8_t)held);
		++len;
	}
	return len;
}

// ---- rule 4: DnsLayer::parseResources ----
// One linked resource of a section the spec asks for, as the sinks get it.
struct Rr
{
	uint32_t offset, name_len, text_len, type, dns_class, ttl, data_len, section;
};

// declared / linked: the four sections' counts as 16-bit fields of one word, section s at bit 16 s (linked <= 300).
struct Walk
{
	uint32_t status, n_rr, name_bytes;
	uint64_t declared, linked;
};

PCPPX_DNS_FN uint32_t count_of(uint64_t packed, uint32_t section)
{
	return (uint32_t)(packed >> (16 * section)) & 0xFFFFu;
}

// d: the layer's L >= 12 + adj bytes. Every linked resource of a section in `sections` goes to s.rr() after its name's
// bytes went to s.put().
template <class Sink>
PCPPX_DNS_FN Walk walk(const uint8_t* d, uint32_t L, uint32_t adj, uint32_t sections, Sink& s)
{
	Walk r{};
	uint32_t sum = 0;
	for (uint32_t k = 0; k < 4; ++k)
	{
		const uint32_t c = be16(d + adj + 4 + 2 * k);
		r.declared |= (uint64_t)c << (16 * k);
		sum += c;
	}
	if (sum > kMaxResources)
	{
		r.status = PCPPX_DNS_TOO_MANY;
		return r;
	}
	uint64_t left = r.declared;  // non-zero while resources are left: its lowest non-zero field is the section
	uint32_t off = kHeader + adj;
	for (uint32_t i = 0; i < sum; ++i)
	{
		const uint32_t sec = (left & 0xFFFFu) != 0 ? 0u : (left & 0xFFFF0000u) != 0 ? 1u : (left & 0xFFFF00000000ull) != 0 ? 2u : 3u;
		const uint64_t one = 1ull << (16 * sec);
		left -= one;
		const NameScan ns = name_scan(d, L, off, adj);
		uint32_t dl = 0, size = ns.name_len + 4;
		if (sec != 0)
		{
			const uint32_t at = off + ns.name_len + 8;
			dl = at >= L - 1 ? 0 : be16(d + at);
			size = ns.name_len + 10 + dl;
		}
		if (off + size > L)
		{
			r.status = PCPPX_DNS_TRUNCATED;
			break;
		}
		r.linked += one;
		if (((sections >> sec) & 1) != 0)
		{
			const uint8_t* f = d + off + ns.name_len;  // type, class (and TTL, data length): inside [off, off + size)
			Rr x;
			x.offset = off;
			x.name_len = ns.name_len;
			x.text_len = ns.ok && ns.name_len != 0 ? name_text(d, L, off, adj, s) : 0;
			x.type = be16(f);
			x.dns_class = be16(f + 2);
			x.ttl = sec == 0 ? 0 : (be16(f + 4) << 16) | be16(f + 6);
			x.data_len = dl;
			x.section = sec;
			s.rr(x);
			++r.n_rr;
			r.name_bytes += x.text_len;
		}
		off += size;
	}
	return r;
}

// the measuring sink
struct CountSink
{
	PCPPX_DNS_FN void put(uint8_t) {}
	PCPPX_DNS_FN void rr(const Rr&) {}
};

// The emitting sink: a message's records from rrs[0] on and its name bytes from position pos of names (when set).
struct EmitSink
{
	pcppx_dns_rr* rrs;
	uint8_t* names;  // or null
	uint64_t pos;    // of the next name byte
	uint32_t msg;    // the message's record number

	PCPPX_DNS_FN void put(uint8_t v)
	{
		if (names != nullptr)
			names[pos] = v;
		++pos;
	}
	PCPPX_DNS_FN void rr(const Rr& x)
	{
		pcppx_dns_rr o;  // built whole and stored once: the record is 8-byte aligned, so the copy is four 64-bit stores
		o.name_pos = pos - x.text_len;
		o.msg = msg;
		o.ttl = x.ttl;
		o.offset = (uint16_t)x.offset;
		o.name_len = (uint16_t)x.name_len;
		o.text_len = (uint16_t)x.text_len;
		o.type = (uint16_t)x.type;
		o.dns_class = (uint16_t)x.dns_class;
		o.data_len = (uint16_t)x.data_len;
		o.data_offset = (uint16_t)(x.section == 0 ? 0 : x.offset + x.name_len + 10);  // <= L
		o.section = (uint8_t)x.section;
		o.reserved = 0;
		*rrs++ = o;
	}
};

// A message's 40-byte record.
PCPPX_DNS_FN void put_msg(pcppx_dns_msg* m, uint64_t first_rr, uint32_t index, const Layer& l, const uint8_t* d,
                          const Walk& w)
{
	pcppx_dns_msg o;
	o.first_rr = first_rr;
	o.index = index;
	o.layer_offset = (uint16_t)l.off;
	o.layer_len = (uint16_t)l.L;
	o.id = (uint16_t)be16(d + l.adj);
	o.flags = (uint16_t)be16(d + l.adj + 2);
	for (uint32_t k = 0; k < 4; ++k)
	{
		o.declared[k] = (uint16_t)count_of(w.declared, k);
		o.linked[k] = (uint16_t)count_of(w.linked, k);
	}
	o.n_rr = (uint16_t)w.n_rr;
	o.adjust = (uint8_t)l.adj;
	o.status = (uint8_t)w.status;
	*m = o;
}
}  // namespace dns
}  // namespace pcppx
