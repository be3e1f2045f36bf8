// pcppx_move.h — device primitives shared by the operators that read or move the packets of a device batch
// (pcppx_select.hip, pcppx_steer.hip, pcppx_bpf.hip, pcppx_defrag.hip, pcppx_frag.hip, pcppx_tlsfp.hip, pcppx_dns.hip, pcppx_http.hip, pcppx_ssl.hip): the descriptor rule, 64-bit
// wave scans, and the pieces of the aligned 16-B copy idiom. Inline device functions only; pcppx_kernels.hip keeps its
// own 32-bit helpers.
#pragma once

#include <hip/hip_runtime.h>

namespace pcppx
{
namespace move
{
// The descriptor rule: packet i is out of bounds (true) when offsets[i] + caplens[i] wraps or exceeds data_len. off = its
// source offset, either way; len = its output length min(caplen, snaplen), snaplen 0 = no limit, written only when the
// packet is in bounds. (The verdict is the bad one on purpose: returning its negation compiles steer's kernels to other
// code; this form leaves them byte for byte what they were with the rule written out in classify.)
__device__ __forceinline__ bool out_of_bounds(const uint64_t* offsets, const uint32_t* caplens, uint64_t data_len,
                                              uint32_t snaplen, uint64_t i, uint64_t& off, uint32_t& len)
{
	off = offsets[i];
	const uint32_t cap = caplens[i];
	const uint64_t end = off + cap;
	if (end < off || end > data_len)
		return true;
	len = (snaplen != 0 && cap > snaplen) ? snaplen : cap;
	return false;
}

__device__ __forceinline__ uint64_t wave_scan_incl(uint64_t v, uint32_t lane)
{
	for (uint32_t o = 1; o < 64; o <<= 1)
	{
		const uint64_t t = __shfl_up(v, o);
		v += lane >= o ? t : 0ull;
	}
	return v;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_xor(v, o);
	return v;
}

// the first packet of 64-packet tile t of this block, which takes block_pk packets
__device__ __forceinline__ uint64_t tile_first(uint32_t block_pk, uint32_t t)
{
	return (uint64_t)blockIdx.x * block_pk + t * 64;
}

// A buffer seen from the 16-B boundary at or below its start: byte position x of the buffer is position
// q = x + shift, which lives at base + q, so that q % 16 = address % 16.
template <typename T>
struct Aligned16
{
	T* base;
	uint32_t shift;
};

template <typename T>
__device__ __forceinline__ Aligned16<T> align16(T* p)
{
	const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15);
	return { p - shift, shift };
}

// bytes sh .. sh+15 of the 32 bytes a:b
__device__ __forceinline__ uint4 funnel16(uint4 a, uint4 b, uint32_t sh)
{
	uint32_t w0 = a.x, w1 = a.y, w2 = a.z, w3 = a.w, w4 = b.x, w5 = b.y;
	if (sh & 8)
	{
		w0 = a.z;
		w1 = a.w;
		w2 = b.x;
		w3 = b.y;
		w4 = b.z;
		w5 = b.w;
	}
	if (sh & 4)
	{
		w0 = w1;
		w1 = w2;
		w2 = w3;
		w3 = w4;
		w4 = w5;
	}
	const uint32_t s = sh & 3;
	return make_uint4(__builtin_amdgcn_alignbyte(w1, w0, s), __builtin_amdgcn_alignbyte(w2, w1, s),
	                  __builtin_amdgcn_alignbyte(w3, w2, s), __builtin_amdgcn_alignbyte(w4, w3, s));
}

// The copy of a wave's 64 independent spans (steer's tiles, defrag's copied packets and fragment pieces): the spans' whole
// destination 16-B chunks form one flattened list that is walked over the 64 lanes; each span's head and tail bytes
// are its own.

// the span (lane number) that owns whole chunk c of the flattened list: the last k <= 63 with cp[k] <= c (cp: the
// exclusive prefix of the spans' whole-chunk counts, ascending; c < cp[64]). Spans without a whole chunk ahead of it are
// passed over; branch-free.
__device__ __forceinline__ uint32_t find_packet(const uint64_t* cp, uint64_t c)
{
	uint32_t k = 0;
#pragma unroll
	for (uint32_t step = 32; step != 0; step >>= 1)
		k = cp[k + step] <= c ? k + step : k;
	return k;
}

// the n (< 16) bytes at source position s (s % 16 = address % 16 from sbase) to destination position q: a span's own
// head or tail, [q, q + n) inside one aligned 16-B chunk. The one or two aligned granules that hold them are read;
// n == 0 reads nothing. Stored in naturally aligned pieces of 1, 2, 4 and 8 B: sizes up to the widest boundary the
// span reaches, then down again -- at most 6 stores, exactly the bytes owned.
__device__ __forceinline__ void copy_edge(const uint8_t* sbase, uint8_t* dbase, uint64_t s, uint64_t q, uint32_t n)
{
	if (n == 0)
		return;
	const uint32_t so = (uint32_t)(s & 15);
	const uint4* g = reinterpret_cast<const uint4*>(sbase + (s & ~15ull));
	const uint4 ga = g[0];
	const uint4 gb = g[so + n > 16 ? 1 : 0];
	const uint4 r = funnel16(ga, gb, so);  // the span's bytes from byte 0
	const uint4 zero = make_uint4(0, 0, 0, 0);
	uint64_t cur = q;
	const uint64_t e = q + n;
	auto put = [&](uint32_t sz) {  // the sz bytes at cur
		const uint4 x = funnel16(r, zero, (uint32_t)(cur - q));
		if (sz == 1)
			dbase[cur] = (uint8_t)x.x;
		else if (sz == 2)
			*reinterpret_cast<uint16_t*>(dbase + cur) = (uint16_t)x.x;
		else if (sz == 4)
			*reinterpret_cast<uint32_t*>(dbase + cur) = x.x;
		else
			*reinterpret_cast<uint2*>(dbase + cur) = make_uint2(x.x, x.y);
		cur += sz;
	};
#pragma unroll
	for (uint32_t sz = 1; sz <= 8; sz <<= 1)  // up: cur becomes a multiple of 2 * sz, or too little is left for sz
		if ((cur & sz) != 0 && cur + sz <= e)
			put(sz);
#pragma unroll
	for (uint32_t sz = 8; sz != 0; sz >>= 1)  // down: cur is a multiple of every size that still fits
		if (cur + sz <= e)
			put(sz);
}
}  // namespace move
}  // namespace pcppx
