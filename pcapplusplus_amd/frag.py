"""A numpy IPv4 fragmenter: what Examples/IPFragUtil does to a capture, for a PacketBatch.

fragment() splits the chosen IPv4 packets of a batch into fragments whose IP payload is at most frag_size bytes
(rounded down to a multiple of 8), following splitIPPacketToFragmentsBySize (Examples/IPFragUtil/main.cpp:153-238):
a packet whose IP payload is not larger than the fragment size is copied as it is; otherwise fragment j carries the
packet's bytes up to the end of its IPv4 header (a trailer behind the IP payload is dropped), then payload bytes
[j * size, min((j + 1) * size, payload)), with the total length, the fragment offset, MF on all but the last fragment
(DF cleared: setIPv4FragmentParams overwrites the word) and the header checksum rewritten. The fragments of a packet
take its place in the batch, in offset order. It is the input side of pcppx_defrag_device's tests and benchmark, and
it is vectorised: no Python loop runs per packet.

The IPv4 header is found behind Ethernet and up to two VLAN tags (the first IPv4 layer of such a packet); other
packets, packets cut short of their IP payload's header, and packets that already are fragments are copied.

fragment6() is the same for the IPv6 packets of a batch (IPFragUtil adds a fragment header behind the existing
extensions), with the fragment ids as an input column: the input side of pcppx_defrag6_device's tests and benchmark.
"""
from __future__ import annotations

import numpy as np

from . import abi
from .pcap import PacketBatch

_CHUNK = 1 << 25  # bytes gathered per step


def locate_ipv4(batch: PacketBatch):
    """(is_v4, ip_off, hdr, payload) per packet: the IPv4 header behind Ethernet and up to two VLAN tags, its length and
    the IP payload's length (the total length field bounds it, and so does the capture). is_v4 is False where there is
    none, where the header is cut short or malformed, or where the link type is not Ethernet."""
    n = batch.n
    off = batch.offsets.astype(np.int64)
    cap = batch.caplens.astype(np.int64)
    zero = np.zeros(n, np.int64)
    if n == 0 or batch.linktype != abi.LINKTYPE_ETHERNET:
        return np.zeros(n, bool), zero, zero.copy(), zero.copy()
    d = batch.data
    last = max(len(d) - 1, 0)

    def u8(pos):
        return d[np.minimum(off + pos, last)].astype(np.int64)

    def be16(pos):
        return (u8(pos) << 8) | u8(pos + 1)

    ip_off = np.full(n, 14, np.int64)
    et = be16(12)
    for _ in range(2):
        tagged = (et == 0x8100) | (et == 0x88A8)
        et = np.where(tagged, be16(ip_off + 2), et)
        ip_off = np.where(tagged, ip_off + 4, ip_off)
    vihl = u8(ip_off)
    hdr = (vihl & 15) * 4
    total = be16(ip_off + 2)
    ok = (et == 0x0800) & (cap >= ip_off + 20) & ((vihl >> 4) == 4) & (hdr >= 20) & (cap >= ip_off + hdr)
    ok &= total >= hdr
    avail = cap - ip_off
    payload = np.where(ok, np.minimum(total, avail) - hdr, 0)
    return ok, np.where(ok, ip_off, 0), np.where(ok, hdr, 0), payload


def _gather(data: np.ndarray, starts: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """The bytes of the ranges [starts[k], starts[k] + lens[k]) back to back."""
    ends = np.cumsum(lens)
    out = np.empty(int(ends[-1]) if len(ends) else 0, np.uint8)
    k0 = 0
    while k0 < len(lens):
        base = int(ends[k0 - 1]) if k0 else 0
        k1 = max(int(np.searchsorted(ends, base + _CHUNK, side="right")), k0 + 1)
        ln = lens[k0:k1]
        pos = ends[k0:k1] - ln - base  # where each range starts in this step's bytes
        idx = np.repeat(starts[k0:k1] - pos, ln) + np.arange(int(ends[k1 - 1]) - base, dtype=np.int64)
        out[base:int(ends[k1 - 1])] = data[idx]
        k0 = k1
    return out


def fragment(batch: PacketBatch, frag_size: int, select=None) -> PacketBatch:
    """The batch with its IPv4 packets split into fragments of at most frag_size payload bytes (a multiple of 8 after
    rounding down; at least 8). select: a boolean mask of the packets to consider (None: all). meta["frag_src"]: the
    source packet of every output packet; meta["frag_no"]: its fragment number (0 for a copied packet);
    meta["frag_count"]: the fragments its source packet was split into (1: copied). timestamps_ns follow the source
    packet; a fragment's frame length is its own length."""
    fs = frag_size // 8 * 8
    if fs < 8:
        raise ValueError("frag_size must be at least 8")
    n = batch.n
    is_v4, ip_off, hdr, pay = locate_ipv4(batch)
    off = batch.offsets.astype(np.int64)
    cap = batch.caplens.astype(np.int64)
    frag_word = np.zeros(n, np.int64)
    if n:
        d, last = batch.data, max(len(batch.data) - 1, 0)
        at = np.minimum(off + ip_off + 6, last)
        frag_word = np.where(is_v4, (d[at].astype(np.int64) << 8) | d[np.minimum(at + 1, last)], 0)
    split = is_v4 & ((frag_word & 0x3FFF) == 0) & (pay > fs)
    if select is not None:
        split &= np.asarray(select, bool)
    count = np.where(split, -(-pay // fs), 1)
    src = np.repeat(np.arange(n, dtype=np.int64), count)
    m = len(src)
    no = np.arange(m, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    is_frag = split[src]
    head = np.where(is_frag, ip_off[src] + hdr[src], cap[src])  # the packet's own bytes, or a fragment's headers
    piece = np.where(is_frag, np.minimum(fs, pay[src] - no * fs), 0)
    starts = np.empty(2 * m, np.int64)
    lens = np.empty(2 * m, np.int64)
    starts[0::2], lens[0::2] = off[src], head
    starts[1::2], lens[1::2] = off[src] + head + no * fs, piece
    out_len = head + piece
    out_off = np.cumsum(out_len) - out_len
    data = _gather(batch.data, starts, lens)
    # the fragments' IPv4 headers: total length, fragment word, checksum
    f = np.nonzero(is_frag)[0]
    if len(f):
        ip = out_off[f] + ip_off[src[f]]
        h = hdr[src[f]]
        tot = h + piece[f]
        word = (no[f] * fs // 8) | np.where(no[f] + 1 < count[src[f]], 0x2000, 0)
        data[ip + 2], data[ip + 3] = (tot >> 8).astype(np.uint8), (tot & 255).astype(np.uint8)
        data[ip + 6], data[ip + 7] = (word >> 8).astype(np.uint8), (word & 255).astype(np.uint8)
        data[ip + 10] = data[ip + 11] = 0
        cols = np.arange(60, dtype=np.int64)
        rows = data[np.minimum(ip[:, None] + cols, len(data) - 1)].astype(np.int64)
        rows[cols[None, :] >= h[:, None]] = 0
        s = (rows[:, 0::2] << 8).sum(axis=1) + rows[:, 1::2].sum(axis=1)
        s = (s & 0xFFFF) + (s >> 16)
        s = (s & 0xFFFF) + (s >> 16)
        ck = ~s & 0xFFFF
        data[ip + 10], data[ip + 11] = (ck >> 8).astype(np.uint8), (ck & 255).astype(np.uint8)
    out = PacketBatch(np.concatenate([data, np.zeros(1, np.uint8)]), out_off.astype(np.uint64),
                      out_len.astype(np.uint32), batch.linktype)
    if batch.timestamps_ns is not None:
        out.timestamps_ns = batch.timestamps_ns[src]
    if batch.frame_lens is not None:
        out.frame_lens = np.where(is_frag, out_len, batch.frame_lens[src]).astype(np.uint32)
    out.meta["frag_src"] = src.astype(np.uint32)
    out.meta["frag_no"] = no.astype(np.uint32)
    out.meta["frag_count"] = count[src].astype(np.uint32)
    return out


_V6_MAX_EXT = 8  # extensions locate_ipv6 walks before it gives a packet up
_L2_LEN = {abi.LINKTYPE_ETHERNET: 14, abi.LINKTYPE_LINUX_SLL: 16}  # the type field is the header's last two bytes


def locate_ipv6(batch: PacketBatch):
    """(is_v6, ip_off, hdr, payload, nh_at, fragmented) per packet: the IPv6 header behind Ethernet (or a Linux cooked
    header) and up to two VLAN tags, the length of its fixed header and extensions (parseExtensions,
    Packet++/src/IPv6Layer.cpp:79-147: types 0,
    43 and 60 are (len8 + 1) * 8 bytes, 44 is 8, 51 is (len8 + 2) * 4), the IP payload's length as the reference's
    layer has it (min(captured, payloadLength + hdr) - hdr, IPv6Layer.cpp:37-39), the packet offset of the next-header
    byte of the last extension (of the fixed header without one) and whether a fragment header is among them. is_v6 is
    False where there is none, where the extensions are cut short or more than _V6_MAX_EXT, or where the link type is
    neither."""
    n = batch.n
    off = batch.offsets.astype(np.int64)
    cap = batch.caplens.astype(np.int64)
    zero = np.zeros(n, np.int64)
    if n == 0 or batch.linktype not in _L2_LEN:
        return np.zeros(n, bool), zero, zero.copy(), zero.copy(), zero.copy(), np.zeros(n, bool)
    d = batch.data
    last = max(len(d) - 1, 0)

    def u8(pos):
        return d[np.clip(off + pos, 0, last)].astype(np.int64)

    def be16(pos):
        return (u8(pos) << 8) | u8(pos + 1)

    ip_off = np.full(n, _L2_LEN[batch.linktype], np.int64)
    et = be16(ip_off - 2)
    for _ in range(2):
        tagged = (et == 0x8100) | (et == 0x88A8)
        et = np.where(tagged, be16(ip_off + 2), et)
        ip_off = np.where(tagged, ip_off + 4, ip_off)
    ok = (et == 0x86DD) & (cap >= ip_off + 40) & ((u8(ip_off) >> 4) == 6)
    nh_at = ip_off + 6
    nh = u8(nh_at)
    hdr = np.full(n, 40, np.int64)
    fragmented = np.zeros(n, bool)
    for _ in range(_V6_MAX_EXT + 1):
        is_ext = ok & np.isin(nh, (0, 43, 44, 51, 60)) & (ip_off + hdr + 2 <= cap)
        len8 = u8(ip_off + hdr + 1)
        ext = np.where(nh == 44, 8, np.where(nh == 51, (len8 + 2) * 4, (len8 + 1) * 8))
        fragmented |= is_ext & (nh == 44)
        nh_at = np.where(is_ext, ip_off + hdr, nh_at)
        nh = np.where(is_ext, u8(ip_off + hdr), nh)
        hdr = np.where(is_ext, hdr + ext, hdr)
    ok &= ~(np.isin(nh, (0, 43, 44, 51, 60)) & (ip_off + hdr + 2 <= cap)) & (cap >= ip_off + hdr)
    payload = np.minimum(cap - ip_off, be16(ip_off + 4) + hdr) - hdr
    ok &= payload >= 0
    keep = lambda a: np.where(ok, a, 0)  # noqa: E731
    return ok, keep(ip_off), keep(hdr), keep(payload), keep(nh_at), fragmented & ok


def fragment6(batch: PacketBatch, frag_size: int, ids, select=None) -> PacketBatch:
    """The batch with its IPv6 packets split into fragments of at most frag_size payload bytes (a multiple of 8 after
    rounding down; at least 8), as Examples/IPFragUtil does (main.cpp:124-128, 153-238): a packet whose IP payload is
    not larger than the fragment size, or that has a fragment header already, is copied as it is; otherwise fragment j
    carries the packet's bytes up to the end of its IPv6 header and extensions, then a fragment header
    (IPv6FragmentationHeader, added behind the last extension: it takes over that extension's next-header value, and
    the extension -- the fixed header without one -- now names type 44), then payload bytes
    [j * size, min((j + 1) * size, payload)); the payload length is rewritten (computeCalculateFields) and a trailer
    behind the IP payload is dropped; the type field ahead of every VLAN tag becomes 0x8100 (computeCalculateFields of
    the layer in front of it: an 802.1ad tag's 0x88A8 is renamed). ids: one 32-bit fragment id per source packet
    (IPFragUtil draws a random one per
    packet; here the caller says, so that the result is a function of the inputs). select, the meta columns,
    timestamps_ns and frame_lens are fragment()'s. IPv4 packets are copied: fragment() splits those."""
    fs = frag_size // 8 * 8
    if fs < 8:
        raise ValueError("frag_size must be at least 8")
    n = batch.n
    ids = np.asarray(ids, dtype=np.int64)
    if ids.shape != (n,):
        raise ValueError("ids: one fragment id per packet")
    is_v6, ip_off, hdr, pay, nh_at, fragmented = locate_ipv6(batch)
    off = batch.offsets.astype(np.int64)
    cap = batch.caplens.astype(np.int64)
    split = is_v6 & ~fragmented & (pay > fs)
    if select is not None:
        split &= np.asarray(select, bool)
    count = np.where(split, -(-pay // fs), 1)
    src = np.repeat(np.arange(n, dtype=np.int64), count)
    m = len(src)
    no = np.arange(m, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    is_frag = split[src]
    head = np.where(is_frag, ip_off[src] + hdr[src], cap[src])  # the packet's own bytes, or a fragment's headers
    ext = np.where(is_frag, 8, 0)                               # the fragment header, filled in below
    piece = np.where(is_frag, np.minimum(fs, pay[src] - no * fs), 0)
    starts = np.empty(3 * m, np.int64)
    lens = np.empty(3 * m, np.int64)
    starts[0::3], lens[0::3] = off[src], head
    starts[1::3], lens[1::3] = off[src], ext  # any 8 bytes of the packet (it has 40 at least)
    starts[2::3], lens[2::3] = off[src] + head + no * fs, piece
    out_len = head + ext + piece
    out_off = np.cumsum(out_len) - out_len
    data = _gather(batch.data, starts, lens)
    f = np.nonzero(is_frag)[0]
    if len(f):
        s = src[f]
        base = out_off[f]
        fh = base + head[f]
        word = (no[f] * fs) | np.where(no[f] + 1 < count[s], 1, 0)
        data[fh] = data[base + nh_at[s]]  # the value the last extension (or the fixed header) named
        data[fh + 1] = 0
        data[fh + 2], data[fh + 3] = (word >> 8).astype(np.uint8), (word & 255).astype(np.uint8)
        for k in range(4):
            data[fh + 4 + k] = ((ids[s] >> (24 - 8 * k)) & 255).astype(np.uint8)
        data[base + nh_at[s]] = 44
        plen = hdr[s] - 40 + 8 + piece[f]
        ip = base + ip_off[s]
        data[ip + 4], data[ip + 5] = (plen >> 8).astype(np.uint8), (plen & 255).astype(np.uint8)
        l2 = _L2_LEN[batch.linktype]
        for t in range(2):
            at = (base + l2 - 2 + 4 * t)[(ip_off[s] - l2) // 4 > t]
            data[at], data[at + 1] = 0x81, 0x00
    out = PacketBatch(np.concatenate([data, np.zeros(1, np.uint8)]), out_off.astype(np.uint64),
                      out_len.astype(np.uint32), batch.linktype)
    if batch.timestamps_ns is not None:
        out.timestamps_ns = batch.timestamps_ns[src]
    if batch.frame_lens is not None:
        out.frame_lens = np.where(is_frag, out_len, batch.frame_lens[src]).astype(np.uint32)
    out.meta["frag_src"] = src.astype(np.uint32)
    out.meta["frag_no"] = no.astype(np.uint32)
    out.meta["frag_count"] = count[src].astype(np.uint32)
    return out
