// pcppx_tlsfp.h — the tlsfp contract of include/pcppx.h as inline functions that pcppx_tlsfp.hip (device) and
// pcppx_tlsfp_ref.cpp (host, also built with a host compiler alone) both compile: the argument rules, the handshake
// layer and message walk (rules 2-4), the fingerprint text as a stream of bytes into a sink (rules 5-7), and MD5
// (rule 8), written from RFC 1321. No reads happen here but through the packet pointer the caller hands in, whose
// bytes [0, caplen) it has found in bounds.
#pragma once

#include <stdint.h>

#include "pcppx.h"
#include "pcppx_args.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PCPPX_TLSFP_FN __host__ __device__ __forceinline__
#else
#define PCPPX_TLSFP_FN inline
#endif

namespace pcppx
{
namespace tlsfp
{
constexpr uint32_t kProtoSSL = 18;  // pcpp::SSL
constexpr uint32_t kHandshake = 22; // SSL_HANDSHAKE

// the argument rules pcppx_tlsfp_device and pcppx_tlsfp_reference share (include/pcppx.h)
inline bool valid_args(const pcppx_batch* b, const pcppx_records* r, uint8_t max_layers, const pcppx_tlsfp_spec* s,
                       const pcppx_tlsfps* o)
{
	if (!valid_source(b, r, max_layers) || s == nullptr || o == nullptr || o->totals == nullptr || o->recs == nullptr)
		return false;
	if (s->client > 1 || s->server > 1 || (s->client == 0 && s->server == 0))
		return false;
	return s->reserved[0] == 0 && s->reserved[1] == 0 && o->reserved == 0;
}

PCPPX_TLSFP_FN uint32_t be16(const uint8_t* p)
{
	return ((uint32_t)p[0] << 8) | p[1];
}

PCPPX_TLSFP_FN bool grease(uint32_t v)
{
	return (v >> 8) == (v & 0xFFu) && (v & 0x0Fu) == 0x0Au;
}

// What rules 2-4 find in an in-bounds packet: its disposition, and for a hello the message's first byte (from the
// packet's first byte), D (the rest of the record from there) and M (the message's length, <= D).
struct Hello
{
	uint32_t msg_off, D, M, disp;
};

// pk: the packet's cap bytes; lay: its ml layer entries; n_layers / flags: of its summary or brief.
PCPPX_TLSFP_FN Hello find_hello(const uint8_t* pk, uint32_t cap, const pcppx_layer* lay, uint32_t n_layers, uint32_t ml,
                                uint32_t flags, bool client, bool server)
{
	Hello h{ 0, 0, 0, PCPPX_TLSFP_NONE };
	const uint32_t nl = n_layers < ml ? n_layers : ml;
	bool found = false;
	uint32_t off = 0, R = 0;
	for (uint32_t k = 0; !found && k < nl; ++k)
	{
		const pcppx_layer L = lay[k];
		if (L.proto != kProtoSSL || L.data_len < 5 || L.hdr_len < 5 || L.hdr_len > L.data_len ||
		    (uint32_t)L.offset + L.data_len > cap)
			continue;
		if (pk[L.offset] != kHandshake)
			continue;
		found = true;
		off = L.offset;
		R = (uint32_t)L.hdr_len - 5;
	}
	if (!found)
	{
		const bool l7 = (flags & PCPPX_F_NEEDS_HOST_L7) != 0 &&
		                ((flags & PCPPX_F_L7_SSL) != 0 || (flags & PCPPX_F_L7_KNOWN) == 0);
		if ((flags & (PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC | PCPPX_F_DEPTH_OVERFLOW)) != 0 ||
		    n_layers > ml || l7)
			h.disp = PCPPX_TLSFP_HOST;
		return h;
	}
	Hello sh = h;  // the first ServerHello, should no ClientHello follow
	for (uint32_t cur = 0; R - cur >= 4;)  // M >= 4: at most R / 4 messages
	{
		const uint32_t D = R - cur;
		const uint8_t* p = pk + off + 5 + cur;
		if (D >= 16 && ((p[0] | p[1] | p[2] | p[3] | p[4]) == 0 || p[1] >= 1))
			break;  // an unknown message takes the rest
		const uint32_t len = 4 + be16(p + 2), M = len < D ? len : D;
		if (client && p[0] == 1)
			return Hello{ off + 5 + cur, D, M, PCPPX_TLSFP_CLIENT };
		if (server && p[0] == 2 && sh.disp == PCPPX_TLSFP_NONE)
			sh = Hello{ off + 5 + cur, D, M, PCPPX_TLSFP_SERVER };
		cur += M;
	}
	return sh;
}

// ---- the text: every byte goes through sink.put(), in order ----
template <class Sink>
PCPPX_TLSFP_FN void put_dec(Sink& s, uint32_t v)  // v <= 65535
{
	if (v >= 10000)
		s.put((uint8_t)('0' + v / 10000));
	if (v >= 1000)
		s.put((uint8_t)('0' + v / 1000 % 10));
	if (v >= 100)
		s.put((uint8_t)('0' + v / 100 % 10));
	if (v >= 10)
		s.put((uint8_t)('0' + v / 10 % 10));
	s.put((uint8_t)('0' + v % 10));
}

template <class Sink>
PCPPX_TLSFP_FN void put_item(Sink& s, bool& first, uint32_t v)
{
	if (!first)
		s.put('-');
	first = false;
	put_dec(s, v);
}

// One extension of the list of rule 5.
struct Ext
{
	uint32_t type, data, len;  // data: its first data byte, from the message's first byte
};

// The extension list at E as a cursor: next() gives the extensions in order.
struct ExtList
{
	uint32_t it, end;
	PCPPX_TLSFP_FN ExtList(const uint8_t* p, uint32_t D, uint32_t M, uint32_t E) : it(0), end(0)
	{
		if (E + 2 > D)
			return;
		it = E + 2;
		const uint32_t e = it + be16(p + E);
		end = e < M ? e : M;
	}
	PCPPX_TLSFP_FN bool next(const uint8_t* p, Ext& x)
	{
		if (it + 4 > end)
			return false;
		x.type = be16(p + it);
		x.len = be16(p + it + 2);
		if (it + 4 + x.len > end)
			return false;
		x.data = it + 4;
		it += 4 + x.len;
		return true;
	}
};

// p: the hello message's first byte; D >= 4 bytes of it are readable. kind: PCPPX_TLSFP_CLIENT / SERVER.
template <class Sink>
PCPPX_TLSFP_FN void hello_text(const uint8_t* p, uint32_t D, uint32_t M, uint32_t kind, Sink& s)
{
	uint32_t sid = 0;
	if (D > 39)
		sid = p[38] < D - 39 ? p[38] : D - 39;
	const uint32_t hv = D < 6 ? 0 : be16(p + 4);
	Ext x;
	if (kind == PCPPX_TLSFP_CLIENT)
	{
		put_dec(s, hv);
		s.put(',');
		const uint32_t cs = 39 + sid, count = cs + 2 > D ? 0 : be16(p + cs) / 2;
		bool first = true;
		for (uint32_t i = 0; i < count && cs + 2 + 2 * (i + 1) <= D; ++i)
		{
			const uint32_t v = be16(p + cs + 2 + 2 * i);
			if (!grease(v))
				put_item(s, first, v);
		}
		s.put(',');
		Ext groups{ 0, 0, 0 }, formats{ 0, 0, 0 };
		bool has_groups = false, has_formats = false;
		first = true;
		for (ExtList l(p, D, M, cs + 2 + 2 * count + 2); l.next(p, x);)
		{
			if (!grease(x.type))
				put_item(s, first, x.type);
			if (x.type == 10 && !has_groups)
			{
				has_groups = true;
				groups = x;
			}
			if (x.type == 11 && !has_formats)
			{
				has_formats = true;
				formats = x;
			}
		}
		s.put(',');
		first = true;
		if (has_groups && groups.len >= 2)
		{
			const uint32_t bytes = be16(p + groups.data);
			if (bytes == groups.len - 2 && (bytes & 1) == 0)
				for (uint32_t j = 0; j < bytes / 2; ++j)
				{
					const uint32_t v = be16(p + groups.data + 2 + 2 * j);
					if (!grease(v))
						put_item(s, first, v);
				}
		}
		s.put(',');
		first = true;
		if (has_formats && formats.len >= 1 && formats.len == (uint32_t)p[formats.data] + 1)
			for (uint32_t j = 1; j < formats.len; ++j)
				put_item(s, first, p[formats.data + j]);
	}
	else
	{
		const uint32_t E = 39 + sid + 3;
		uint32_t version = hv;
		for (ExtList l(p, D, M, E); l.next(p, x);)
			if (x.type == 43)  // the first one decides
			{
				if (x.len == 2)
					version = be16(p + x.data);
				else if (x.len == 3 && p[x.data] == 2)
					version = be16(p + x.data + 1);
				break;
			}
		put_dec(s, version);
		s.put(',');
		put_dec(s, 39 + sid + 2 > D ? 0 : be16(p + 39 + sid));
		s.put(',');
		bool first = true;
		for (ExtList l(p, D, M, E); l.next(p, x);)
			put_item(s, first, x.type);
	}
}

// the measuring sink
struct CountSink
{
	uint32_t len = 0;
	PCPPX_TLSFP_FN void put(uint8_t)
	{
		++len;
	}
};

// ---- MD5 (RFC 1321) ----
PCPPX_TLSFP_FN uint32_t rotl(uint32_t v, uint32_t s)
{
	return (v << s) | (v >> (32 - s));
}

// one 64-byte block m (16 little-endian words) into the state
PCPPX_TLSFP_FN void md5_block(uint32_t& a0, uint32_t& b0, uint32_t& c0, uint32_t& d0, const uint32_t (&m)[16])
{
	// T[i] = floor(2^32 * abs(sin(i + 1))) and the per-round shifts (RFC 1321, 3.4); compile-time in the unrolled loop
	const uint32_t T[64] = {
		0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
		0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
		0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
		0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
		0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
		0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
		0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
		0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391,
	};
	const uint32_t S[16] = { 7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21 };
	uint32_t a = a0, b = b0, c = c0, d = d0;
#if defined(__clang__)
#pragma unroll
#endif
	for (uint32_t i = 0; i < 64; ++i)
	{
		uint32_t f, g;
		if (i < 16)
		{
			f = (b & c) | (~b & d);
			g = i;
		}
		else if (i < 32)
		{
			f = (d & b) | (~d & c);
			g = (5 * i + 1) & 15;
		}
		else if (i < 48)
		{
			f = b ^ c ^ d;
			g = (3 * i + 5) & 15;
		}
		else
		{
			f = c ^ (b | ~d);
			g = (7 * i) & 15;
		}
		const uint32_t t = d;
		d = c;
		c = b;
		b = b + rotl(a + f + T[i] + m[g], S[(i >> 4) * 4 + (i & 3)]);
		a = t;
	}
	a0 += a;
	b0 += b;
	c0 += c;
	d0 += d;
}

// The emitting sink: every byte goes to `text` (when set) and into the MD5 of the text. The 64-byte block is kept as
// 16 words at blk[w * Stride]: on the device a column of an LDS array shared by the block's threads (word w of thread
// t at w * threads + t: neighbouring lanes hit different banks, and no register array is indexed at run time), on
// the host 16 words of its own.
template <uint32_t Stride>
struct Md5Sink
{
	uint32_t* blk;
	uint8_t* text;  // the text's first byte, or null
	uint32_t a, b, c, d, word, len;

	PCPPX_TLSFP_FN Md5Sink(uint32_t* block, uint8_t* out)
	    : blk(block), text(out), a(0x67452301), b(0xefcdab89), c(0x98badcfe), d(0x10325476), word(0), len(0)
	{}

	PCPPX_TLSFP_FN void push(uint8_t v)  // into the digest alone
	{
		word |= (uint32_t)v << (8 * (len & 3));
		if ((len & 3) == 3)
		{
			blk[((len >> 2) & 15) * Stride] = word;
			word = 0;
			if ((len & 63) == 63)
			{
				uint32_t m[16];
#if defined(__clang__)
#pragma unroll
#endif
				for (uint32_t w = 0; w < 16; ++w)
					m[w] = blk[w * Stride];
				md5_block(a, b, c, d, m);
			}
		}
		++len;
	}

	PCPPX_TLSFP_FN void put(uint8_t v)
	{
		if (text != nullptr)
			text[len] = v;
		push(v);
	}

	// padding and the length word; the digest's 16 bytes as four little-endian words. len is the text's length before.
	PCPPX_TLSFP_FN void finish(uint32_t (&digest)[4])
	{
		const uint64_t bits = (uint64_t)len * 8;
		push(0x80);
		while ((len & 63) != 56)
			push(0);
		for (uint32_t k = 0; k < 8; ++k)
			push((uint8_t)(bits >> (8 * k)));
		digest[0] = a;
		digest[1] = b;
		digest[2] = c;
		digest[3] = d;
	}
};
}  // namespace tlsfp
}  // namespace pcppx
