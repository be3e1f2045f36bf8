"""Checksum edge cases and an independent RFC 1071 reference for them (host only; tests/test_checksums.py).

Every packet is built here from fixed addresses, ports 1234 / 4321 (no L7 dissector triggers on them) and seeded
payloads, so the generator knows where each layer starts and computes the expected values from those offsets, not
from a parse: the Internet checksum in plain Python ints (RFC 1071: the big-endian 16-bit words of the pseudo header
and the L4 bytes with the checksum field zeroed, an odd last byte zero-padded, end-around carry, inverted; UDP maps
0 to 0xFFFF) and the IPv4 header checksum over min(IHL * 4, data length) bytes. The pseudo-header length is the
captured L4 length where the capture is shorter than the IP length; the pseudo header is that of the IP layer in
front of the L4 layer, the IPv4 header checksum that of the chain's first IPv4 layer. Nothing here calls the
restatement (oracle/) or the engine package's arithmetic: PacketBatch is only the container the engine takes.

Sets (each a list of CaseBatch, one engine launch each):
  S1  payload length x start alignment, stored checksums valid
  S2  residue edges: computed checksums steered to 0x0000 / 0x0001 / 0xFFFE / 0x00FF / 0xFF00 / 0x8000 and the
      0x0000 / 0xFFFF aliases that must not verify
  S3  chain shapes: Ethernet padding, truncated captures, VLAN / MPLS / IPv4 options pushing the IPv4 and L4 headers
      across the ends of the 96-B and 144-B header windows, GRE with an inner IP layer
  S4  batch structure: partial tiles, dead descriptors inside a streaming tile, tiles too sparse to stream, the
      stream criterion on both sides, sums near and past 2^32, descriptors sharing bytes
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from pcapplusplus_amd.pcap import PacketBatch

FAMILIES = ("IPv4/TCP", "IPv4/UDP", "IPv6/TCP", "IPv6/UDP")
MAC_DST, MAC_SRC = bytes.fromhex("021122334455"), bytes.fromhex("0266778899aa")
V4_SRC, V4_DST = bytes([10, 1, 2, 3]), bytes([192, 168, 9, 1])
V4_OUT_SRC, V4_OUT_DST = bytes([172, 16, 0, 9]), bytes([172, 16, 200, 77])  # the GRE carrier
V6_SRC = bytes.fromhex("20010db885a3000000008a2e03707334")
V6_DST = bytes.fromhex("fe80000000000000021122fffe334455")
SPORT, DPORT = 1234, 4321
FILL = 0xCC  # gap bytes between packets
TILE = 64    # packets per wave of the tile kernel
DEAD_BAD_DESC, DEAD_EMPTY, DEAD_OVERSIZE = 1, 2, 3

EXPECT_DTYPE = np.dtype([("live", "?"), ("dead", "u1"), ("l4_calc", "<u2"), ("l4_stored", "<u2"), ("l4_ok", "?"),
                         ("has_ip4", "?"), ("ip_calc", "<u2"), ("ip_stored", "<u2"), ("ip_ok", "?"), ("trailer", "?"),
                         ("align", "u1"), ("length", "<u4")])


# ---------------------------------------------------------------- the reference (RFC 1071, plain ints)
def ones_sum(data: bytes) -> int:
    """End-around-carry sum of the big-endian 16-bit words of data (an odd last byte zero-padded): 0..0xFFFF."""
    if len(data) & 1:
        data = data + b"\0"
    s = sum(struct.unpack(f">{len(data) // 2}H", data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def inet_checksum(data: bytes) -> int:
    return ~ones_sum(data) & 0xFFFF


def pseudo_header(ipver: int, src: bytes, dst: bytes, proto: int, length: int) -> bytes:
    if ipver == 4:
        return src + dst + bytes([0, proto]) + struct.pack(">H", length)
    return src + dst + struct.pack(">I", length) + bytes([0, 0, 0, proto])


def l4_checksum(ipver: int, src: bytes, dst: bytes, proto: int, seg: bytes, raw: bool = False) -> int:
    """The TCP (6) / UDP (17) checksum of the L4 bytes seg (header + payload as captured), its field zeroed; raw: without
    UDP's 0 -> 0xFFFF."""
    at = 16 if proto == 6 else 6
    assert len(seg) >= at + 2
    c = inet_checksum(pseudo_header(ipver, src, dst, proto, len(seg)) + seg[:at] + b"\0\0" + seg[at + 2:])
    return 0xFFFF if (proto == 17 and c == 0 and not raw) else c


def ipv4_header_checksum(hdr: bytes) -> int:
    return inet_checksum(hdr[:10] + b"\0\0" + hdr[12:])


# ---------------------------------------------------------------- packets
@dataclass
class Pkt:
    data: bytes
    family: str
    length: int          # L4 payload bytes built (before any cut)
    note: str
    l4_calc: int
    l4_stored: int
    has_ip4: bool
    ip_calc: int
    ip_stored: int
    trailer: bool
    l4_off: int


def ipv4_header(proto: int, payload_len: int, ihl: int, src: bytes, dst: bytes, ident: int, stored: int | None) -> bytes:
    h = bytearray(b"\x01" * (ihl * 4))  # options: NOPs
    h[0] = 0x40 | ihl
    h[1] = 0
    struct.pack_into(">HHHBBH", h, 2, ihl * 4 + payload_len, ident, 0x4000, 64, proto, 0)
    h[12:16], h[16:20] = src, dst
    struct.pack_into(">H", h, 10, ipv4_header_checksum(bytes(h)) if stored is None else stored)
    return bytes(h)


def ipv6_header(nh: int, payload_len: int) -> bytes:
    return struct.pack(">IHBB", 0x60000000, payload_len, nh, 64) + V6_SRC + V6_DST


def build(family: str, payload: bytes, *, ihl: int = 5, vlans: int = 0, mpls: int = 0, gre: bool = False,
          pad: bytes = b"", cut: int = 0, l4_stored: int | None = None, ip_stored: int | None = None,
          ip_id: int = 7, note: str = "") -> Pkt:
    """Ethernet [VLAN x vlans] [MPLS x mpls] [IPv4(IHL 6) GREv0] IP L4 payload [pad], the last `cut` bytes not captured.
    ihl: the IHL of the IPv4 layer in front of the L4 layer; l4_stored / ip_stored: the stored checksum fields (None: the
    valid checksum of the whole datagram; ip_stored and ip_id belong to the chain's first IPv4 layer)."""
    ipver = 4 if family.startswith("IPv4") else 6
    proto = 6 if family.endswith("TCP") else 17
    if proto == 6:
        hdr, at = struct.pack(">HHIIBBHHH", SPORT, DPORT, 0x01020304, 0x05060708, 5 << 4, 0x18, 4096, 0, 0), 16
    else:
        hdr, at = struct.pack(">HHHH", SPORT, DPORT, 8 + len(payload), 0), 6
    src, dst = (V4_SRC, V4_DST) if ipver == 4 else (V6_SRC, V6_DST)
    seg = hdr + payload
    st = l4_checksum(ipver, src, dst, proto, seg) if l4_stored is None else l4_stored
    seg = seg[:at] + struct.pack(">H", st) + seg[at + 2:]
    inner_first = ipver == 4 and not gre
    if ipver == 4:
        ip = ipv4_header(proto, len(seg), ihl, src, dst, ip_id if inner_first else 9, ip_stored if inner_first else None)
    else:
        ip = ipv6_header(proto, len(seg))
    et_ip = 0x0800 if (gre or ipver == 4) else 0x86DD
    types = [0x8100] * vlans + [0x8847 if mpls else et_ip]
    l2 = MAC_DST + MAC_SRC + struct.pack(">H", types[0])
    l2 += b"".join(struct.pack(">HH", 100 + k, types[k + 1]) for k in range(vlans))
    l2 += b"".join(struct.pack(">I", (1000 + k) << 12 | (1 if k == mpls - 1 else 0) << 8 | 64) for k in range(mpls))
    if gre:
        inner = ip + seg
        g = struct.pack(">HH", 0, 0x0800 if ipver == 4 else 0x86DD)
        outer = ipv4_header(47, len(g) + len(inner), 6, V4_OUT_SRC, V4_OUT_DST, ip_id, ip_stored)
        body, first4, l4_off = outer + g + inner, len(l2), len(l2) + len(outer) + len(g) + len(ip)
    else:
        body, first4, l4_off = ip + seg, (len(l2) if ipver == 4 else None), len(l2) + len(ip)
    full = l2 + body + pad
    assert 0 <= cut <= len(payload) + len(pad) and not (cut and gre)
    data = full[: len(full) - cut]
    cap = len(data)
    # expected values, from the offsets known here
    seg_cap = data[l4_off: min(cap, l4_off + len(seg))]
    l4_calc = l4_checksum(ipver, src, dst, proto, seg_cap)
    has4 = first4 is not None
    ip_calc = ip_st = 0
    if has4:
        hl4 = (data[first4] & 0xF) * 4
        total = struct.unpack_from(">H", data, first4 + 2)[0]
        hl = min(hl4, min(total, cap - first4))
        ip_calc = ipv4_header_checksum(data[first4: first4 + hl])
        ip_st = struct.unpack_from(">H", data, first4 + 10)[0]
    return Pkt(data, family, len(payload), note, l4_calc, st, has4, ip_calc, ip_st, cap > len(l2) + len(body), l4_off)


def steer_l4(family: str, payload: bytes, target: int, **kw) -> bytes:
    """payload with its last aligned 16-bit word replaced so that the (unmapped) L4 checksum of the whole datagram is
    `target` (0x0000..0xFFFE: an all-ones sum, i.e. 0xFFFF before UDP's mapping, cannot occur: the protocol byte of the
    pseudo header is not zero)."""
    assert len(payload) >= 2 and 0 <= target < 0xFFFF
    at = 2 * (len(payload) // 2 - 1)
    base = payload[:at] + b"\0\0" + payload[at + 2:]
    ipver, proto = (4 if family.startswith("IPv4") else 6), (6 if family.endswith("TCP") else 17)
    src, dst = (V4_SRC, V4_DST) if ipver == 4 else (V6_SRC, V6_DST)
    p0 = build(family, base, **kw)
    seg0 = p0.data[p0.l4_off: p0.l4_off + (20 if proto == 6 else 8) + len(base)]
    s0 = ~l4_checksum(ipver, src, dst, proto, seg0, raw=True) & 0xFFFF  # folded sum with the word at 0: 1..0xFFFF
    want = ~target & 0xFFFF                                              # folded sum asked for: 1..0xFFFF
    w = (want - s0) % 65535  # both in 1..0xFFFF and congruent mod 65535 afterwards, hence equal
    out = base[:at] + struct.pack(">H", w) + base[at + 2:]
    p1 = build(family, out, **kw)
    seg1 = p1.data[p1.l4_off: p1.l4_off + (20 if proto == 6 else 8) + len(out)]
    assert l4_checksum(ipver, src, dst, proto, seg1, raw=True) == target
    return out


def steer_ip_id(family: str, payload: bytes, target: int, **kw) -> int:
    """The IPv4 identification that makes the header checksum `target` (not 0xFFFF: the version nibble is not zero)."""
    p0 = build(family, payload, ip_id=0, **kw)
    assert p0.has_ip4 and 0 <= target < 0xFFFF
    s0 = ~p0.ip_calc & 0xFFFF
    ident = ((~target & 0xFFFF) - s0) % 65535
    assert build(family, payload, ip_id=ident, **kw).ip_calc == target
    return ident


# ---------------------------------------------------------------- batches
@dataclass
class CaseBatch:
    name: str
    batch: PacketBatch
    expect: np.ndarray            # EXPECT_DTYPE per descriptor
    labels: list[str]             # per descriptor: family and what the case is
    stream: list[bool] | None = None   # per 64-descriptor tile: whether the tile is meant to take the span stream
    alone: "CaseBatch | None" = None   # the live packets of a batch with dead descriptors, by themselves
    meta: dict = field(default_factory=dict)

    def describe(self, i: int) -> str:
        e = self.expect[i]
        return (f"{self.name} #{i} [{self.labels[i]}] start%16={int(e['align'])} payload={int(e['length'])} "
                f"caplen={int(self.batch.caplens[i])}")


def expect_row(p: Pkt, offset: int) -> tuple:
    return (True, 0, p.l4_calc, p.l4_stored, p.l4_calc == p.l4_stored, p.has_ip4, p.ip_calc, p.ip_stored,
            p.has_ip4 and p.ip_calc == p.ip_stored, p.trailer, offset % 16, p.length)


def place(name: str, pkts: list[Pkt], aligns=None, offsets=None, tail: int = 16, order=None) -> CaseBatch:
    """Lay packets into one buffer of FILL bytes: at explicit byte offsets, or packed with the smallest gap that puts
    packet k's first byte at aligns[k] mod 16. tail: FILL bytes kept after the last packet (16: every 16-B chunk a
    kernel touches lies inside the buffer). order: descriptor order as indices into pkts (default: as placed)."""
    if offsets is None:
        offsets, pos = [], 0
        for p, a in zip(pkts, aligns):
            pos += (a - pos) % 16
            offsets.append(pos)
            pos += len(p.data)
    end = max(o + len(p.data) for o, p in zip(offsets, pkts))
    data = np.full(end + tail, FILL, dtype=np.uint8)
    for o, p in zip(offsets, pkts):
        data[o:o + len(p.data)] = np.frombuffer(p.data, dtype=np.uint8)
    order = list(range(len(pkts))) if order is None else list(order)
    offs = np.array([offsets[k] for k in order], dtype=np.uint64)
    caps = np.array([len(pkts[k].data) for k in order], dtype=np.uint32)
    exp = np.array([expect_row(pkts[k], offsets[k]) for k in order], dtype=EXPECT_DTYPE)
    labels = [f"{pkts[k].family} {pkts[k].note}".strip() for k in order]
    return CaseBatch(name, PacketBatch(data, offs, caps), exp, labels)


def tile_span(batch: PacketBatch, t: int) -> tuple[int, int, int]:
    """(smin, emax, wire) of tile t as the tile kernel takes them from the descriptors (relative to a 16-B aligned
    buffer): the 16-B rounded extent of its live packets and the sum of their captured lengths."""
    lo, hi = t * TILE, min((t + 1) * TILE, batch.n)
    off = batch.offsets[lo:hi].astype(np.int64)
    cap = batch.caplens[lo:hi].astype(np.int64)
    live = (off + cap <= batch.data.nbytes) & (cap <= 65535) & (cap > 0)
    off, cap = off[live], cap[live]
    return int((off & ~15).min()), int(((off + cap + 15) & ~15).max()), int(cap.sum())


def tile_streams(batch: PacketBatch, t: int) -> bool:
    smin, emax, wire = tile_span(batch, t)
    return emax > smin and emax - smin <= 2 * wire + 65536


# ---------------------------------------------------------------- S1
S1_LENGTHS = tuple(range(0, 97)) + (127, 128, 129, 255, 256, 257, 1459, 1460, 1461)


@lru_cache(maxsize=None)
def s1_packets() -> tuple[tuple[Pkt, ...], tuple[int, ...]]:
    """Every payload length x family x start alignment, IHL cycling 5..15, in a seeded order (so that a tile mixes lengths
    and families, and the first packets S4 reuses are varied)."""
    rng = np.random.default_rng(1071)
    combos = [(ln, f, a) for ln in S1_LENGTHS for f in FAMILIES for a in range(16)]
    pkts, aligns = [], []
    for k, j in enumerate(rng.permutation(len(combos))):
        ln, f, a = combos[int(j)]
        ihl = 5 + k % 11
        pkts.append(build(f, rng.bytes(ln), ihl=ihl, note=f"ihl={ihl}" if f.startswith("IPv4") else ""))
        aligns.append(a)
    return tuple(pkts), tuple(aligns)


@lru_cache(maxsize=None)
def s1() -> list[CaseBatch]:
    pkts, aligns = s1_packets()
    return [place("S1", list(pkts), aligns)]


# ---------------------------------------------------------------- S2
S2_LENGTHS = (2, 3, 17, 64, 65, 300)
S2_TARGETS = (0x0000, 0x0001, 0xFFFE, 0x00FF, 0xFF00, 0x8000)


@lru_cache(maxsize=None)
def s2() -> list[CaseBatch]:
    rng = np.random.default_rng(65535)
    pkts = []
    for f in FAMILIES:
        udp = f.endswith("UDP")
        for ln in S2_LENGTHS:
            for fill in ("random", "zeros", "ones"):
                pay = rng.bytes(ln) if fill == "random" else bytes([0x00 if fill == "zeros" else 0xFF]) * ln
                for tgt in S2_TARGETS:
                    p = build(f, steer_l4(f, pay, tgt), note=f"{fill} steered to {tgt:#06x}")
                    assert p.l4_calc == (0xFFFF if (udp and tgt == 0) else tgt) and p.l4_stored == p.l4_calc
                    pkts.append(p)
                # the aliases of zero: the stored field holds the other representation, and must not verify
                z = steer_l4(f, pay, 0)
                p = build(f, z, l4_stored=0x0000 if udp else 0xFFFF, note=f"{fill} alias of zero")
                assert p.l4_calc == (0xFFFF if udp else 0x0000) and p.l4_calc != p.l4_stored
                pkts.append(p)
        if f.startswith("IPv4"):
            # the IPv4 header checksum steered to 0x0000 through the identification: stored 0x0000 verifies, stored 0xFFFF
            # (the same value mod 65535) does not; and a stored 0x0000 / 0xFFFF against a header whose checksum is 0x0001 /
            # 0xFFFE (a computed 0xFFFF cannot occur)
            for ln in S2_LENGTHS:
                pay = rng.bytes(ln)
                for tgt, stored in ((0x0000, 0x0000), (0x0000, 0xFFFF), (0x0001, 0x0000), (0xFFFE, 0xFFFF)):
                    ident = steer_ip_id(f, pay, tgt)
                    p = build(f, pay, ip_id=ident, ip_stored=stored, note=f"ip steered to {tgt:#06x} stored {stored:#06x}")
                    assert p.ip_calc == tgt and p.ip_stored == stored
                    pkts.append(p)
    both, aligns = [], []
    for k, p in enumerate(pkts):  # each case at one even and one odd start address
        both += [p, p]
        aligns += [2 * (k % 8), 2 * ((k + 3) % 8) + 1]
    return [place("S2", both, aligns)]


# ---------------------------------------------------------------- S3
@lru_cache(maxsize=None)
def s3() -> list[CaseBatch]:
    rng = np.random.default_rng(144)
    pkts = []
    for f in FAMILIES:  # (a) Ethernet padding after the datagram: a trailer, not part of the sum
        for npad in range(1, 6):
            for ln in (0, 1, 7, 33):
                pkts.append(build(f, rng.bytes(ln), pad=b"\xa5" * npad, note=f"pad={npad}"))
    # (b) captures cut short. A cut that would reach into the L4 header (290 of a 40- or 100-byte payload) is left
    # out: such a capture has no whole L4 header to sum (and 290 bytes is more than the whole 40-byte-payload packet)
    for f in FAMILIES:
        for ln in (40, 100, 300):
            for cut in (1, 7, 33, 290):
                if cut <= ln:
                    pkts.append(build(f, rng.bytes(ln), cut=cut, note=f"cut={cut}"))
    # (c) tags, labels and IPv4 options moving the IPv4 and L4 headers over the ends of the 96-B / 144-B header windows
    for vl in range(3):
        for ml in range(4):
            for ihl in (5, 8, 12, 15):
                for f in ("IPv4/TCP", "IPv4/UDP"):
                    pkts.append(build(f, rng.bytes(37), ihl=ihl, vlans=vl, mpls=ml, note=f"vlan={vl} mpls={ml} ihl={ihl}"))
    for f in FAMILIES:  # (d) GREv0 behind an IPv4 header with options: the pseudo header is the inner IP layer's
        pkts.append(build(f, rng.bytes(29), gre=True, note="gre"))
    rep, aligns = [], []
    for p in pkts:
        rep += [p] * 16
        aligns += list(range(16))
    return [place("S3", rep, aligns)]


# ---------------------------------------------------------------- S4
def _dead_lanes(cb: CaseBatch) -> CaseBatch:
    """Every 4th descriptor replaced in turn by one the engine does not parse: past the buffer, empty, oversize."""
    b = cb.batch
    offs, caps, exp = b.offsets.copy(), b.caplens.copy(), cb.expect.copy()
    labels = list(cb.labels)
    for n, j in enumerate(range(3, b.n, 4)):
        kind = (DEAD_BAD_DESC, DEAD_EMPTY, DEAD_OVERSIZE)[n % 3]
        if kind == DEAD_BAD_DESC:
            offs[j], caps[j] = b.data.nbytes - 8, 64
        else:
            caps[j] = 0 if kind == DEAD_EMPTY else 65536
        assert kind != DEAD_OVERSIZE or int(offs[j]) + 65536 <= b.data.nbytes
        exp[j] = np.zeros(1, EXPECT_DTYPE)[0]
        exp[j]["dead"] = kind
        labels[j] = ("", "BAD_DESC", "empty", "OVERSIZE")[kind]
    live = np.nonzero(exp["live"])[0]
    alone = CaseBatch(cb.name + "/alone", PacketBatch(b.data, offs[live].copy(), caps[live].copy()), exp[live].copy(),
                      [labels[int(i)] for i in live])
    return CaseBatch(cb.name, PacketBatch(b.data, offs, caps), exp, labels, alone=alone, meta={"live": live})


def _sized(rng, k: int, total: int, fill: int | None = None) -> Pkt:
    """A packet of family k % 4 with `total` captured bytes (or its headers, if they are longer)."""
    f = FAMILIES[k % 4]
    hdrs = 14 + (20 if f.startswith("IPv4") else 40) + (20 if f.endswith("TCP") else 8)
    ln = max(0, total - hdrs)
    return build(f, rng.bytes(ln) if fill is None else bytes([fill]) * ln, note=f"size={hdrs + ln}")


@lru_cache(maxsize=None)
def s4() -> list[CaseBatch]:
    rng = np.random.default_rng(4099)
    pkts, aligns = s1_packets()
    out = []
    # (a) partial tiles
    for n in (1, 63, 64, 65, 129):
        out.append(place(f"S4a/n={n}", list(pkts[:n]), aligns[:n]))
    # (b) dead lanes in two streaming tiles (the buffer keeps 64 KiB + behind them for the oversize descriptors)
    cb = _dead_lanes(place("S4b/dead-lanes", list(pkts[129:257]), aligns[129:257], tail=65536 + 64))
    cb.stream = [True, True]
    out.append(cb)
    # (c) tiles that cannot stream: a 4099-B stride (odd: every alignment), lengths 60..1514, forwards and backwards
    sizes = [60, 1514] + [int(x) for x in rng.integers(60, 1515, 126)]
    sparse = [_sized(rng, k, s) for k, s in enumerate(sizes)]
    offs = [4099 * k for k in range(128)]
    for name, order in (("S4c/stride-4099", range(128)), ("S4c/stride-4099-reversed", range(127, -1, -1))):
        cb = place(name, sparse, offsets=offs, order=order)
        cb.stream = [False, False]
        out.append(cb)
    # (d) the stream criterion met exactly (tile 0) and missed by one chunk (tile 1): 64 packets, one gap after the 32nd
    tile = list(pkts[300:363])
    rest = [p for p in pkts[363:] if (sum(len(q.data) for q in tile) + len(p.data)) % 8 == 0]
    tile.append(rest[0])  # the tile's captured bytes a multiple of 8: 2 * wire + 65536 is then a multiple of 16
    wire = sum(len(p.data) for p in tile)
    offs, base = [], 0
    for extra in (0, 16):
        head = sum(len(p.data) for p in tile[:32])
        back = sum(len(p.data) for p in tile[32:])
        span = 2 * wire + 65536 + extra          # emax - smin asked for; smin = base (16-B aligned)
        o, pos = [], base
        for p in tile[:32]:
            o.append(pos)
            pos += len(p.data)
        pos = base + span - back - 5             # the last packet ends 5 B before emax: second half on odd addresses
        assert pos >= base + head
        for p in tile[32:]:
            o.append(pos)
            pos += len(p.data)
        offs += o
        base = (pos + 15 + 16) & ~15
    cb = place("S4d/stream-criterion", tile + tile, offsets=offs)
    cb.stream = [True, False]
    cb.meta["wire"] = wire
    out.append(cb)
    # (e) large sums: 64 x 9000 B of 0xFF packed (the streamed prefix passes 2^32), the same at a stride too sparse to
    # stream (whole-chunk sums from memory), and one 65,535-B capture of 0xFF per family (a u32 sum just under 2^32)
    jumbo = [build(("IPv4/TCP", "IPv6/TCP")[k % 2], b"\xff" * (9000 - 54 - 20 * (k % 2)), note="9000 B of 0xFF")
             for k in range(64)]
    assert all(len(p.data) == 9000 for p in jumbo)
    stride = 9000 + 3 * 4099  # odd, and 64 strides exceed 2 * 64 * 9000 + 65536
    big = []
    for f in FAMILIES:
        hdrs = 14 + (20 if f.startswith("IPv4") else 40) + (20 if f.endswith("TCP") else 8)
        big.append(build(f, b"\xff" * (65535 - hdrs), note="65535 B of 0xFF"))
    assert all(len(p.data) == 65535 for p in big)
    base2 = (64 * 9000 + 15) & ~15
    base3 = (base2 + 63 * stride + 9000 + 15) & ~15
    offs = [9000 * k for k in range(64)] + [base2 + 5 + stride * k for k in range(64)]
    pos = base3 + 3
    for p in big:
        offs.append(pos)
        pos += 65535
    cb = place("S4e/large-sums", jumbo + jumbo + big, offsets=offs)
    cb.stream = [True, False, True]
    out.append(cb)
    # (f) descriptors sharing bytes, a tile in descending address order, one long packet ahead of 63 short ones
    one = build("IPv4/TCP", rng.bytes(1514 - 54), note="shared")
    cb = place("S4f/one-packet-64-times", [one], offsets=[7], order=[0] * 64)
    cb.stream = [True]
    out.append(cb)
    cb = place("S4f/descending", list(pkts[400:464]), aligns[400:464], order=range(63, -1, -1))
    cb.stream = [True]
    out.append(cb)
    mixed = [build("IPv6/UDP", rng.bytes(9000 - 62), note="9000 B")] + [_sized(rng, k, 64) for k in range(63)]
    cb = place("S4f/long-then-short", mixed, [k % 16 for k in range(64)])
    cb.stream = [True]
    out.append(cb)
    return out


SETS = {"S1": s1, "S2": s2, "S3": s3, "S4": s4}
