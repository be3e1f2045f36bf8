"""Layouts for batches, spans and outputs on both sides of 2^32 (host only, pure numpy; tests/test_wide_offsets.py).

Two lines cut a buffer of 4 GiB and more: the offset line (packet offset 2^32: whatever keeps an offset, a position or
data_len in 32 bits breaks there) and the address line (the data offset whose device address is a multiple of 2^32:
whatever does address arithmetic on the low dword alone breaks there). layout() picks, from the address an allocation
got, the view into it that puts both lines where the packets are; stages() lays packets around the two lines.

Only one packet can lie across a line, so the cases come as stages: each stage is a few small extents of bytes to put
into the (otherwise unwritten) wide buffer, and descriptors over them, one or more whole 64-packet tiles per line. The
same extents packed into a small host array with the descriptors rebased are the compact batch the expected records
come from: no record field depends on a packet's absolute offset.

period() is the source of the outputs that pass 2^32: P descriptors over a 1 MiB block, repeated R times on the device.
By stability the output of R periods is R shifted copies of one period's output, which pcppx_select_reference /
pcppx_steer_reference give on the CPU.
"""
from __future__ import annotations

import bisect
from dataclasses import dataclass, field
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import checksum_cases as cc
from pcapplusplus_amd.pcap import PacketBatch

LINE = 1 << 32
MIB = 1 << 20
RAW_BYTES = LINE + (1 << 27)   # the wide allocation
SLACK = 64                     # bytes kept unused at both ends of the allocation
MARGIN = 16 * MIB              # both lines at least this far from each other and from the ends of the data
MIN_DATA = LINE + 32 * MIB
TILE = cc.TILE
SPARSE_STRIDE = MIB + 4099     # odd: every alignment
SPARSE_REACH = 7               # sparse tiles: spots at -7 .. +7 strides around the line


# ---------------------------------------------------------------- where the lines fall
@dataclass(frozen=True)
class Layout:
    pad: int        # data = raw[pad : pad + data_len]
    data_len: int
    addr_line: int  # data offset of the address line the stages are built around
    mis: int        # data's address mod 16

    @property
    def lines(self) -> tuple[int, int]:
        return (LINE, self.addr_line)


def layout(raw_ptr: int, mis: int, raw_bytes: int = RAW_BYTES) -> Layout:
    """The view of an allocation at address raw_ptr that starts `mis` bytes past a 16-B boundary, keeps SLACK bytes at
    both ends, and has an address line at least MARGIN away from its ends and from offset 2^32."""
    r = (-raw_ptr) % LINE  # raw offset of the first address line (a second one lies 2^32 further, if inside)
    lo = SLACK
    if r < lo + MARGIN + 16:       # too close to the front (a 4 GiB-aligned allocation has r = 0): take the second one
        r += LINE
    lo = max(lo, r - (LINE - MARGIN))  # ... or too close to offset 2^32 from below: start later
    pad = lo + (mis - (raw_ptr + lo)) % 16
    lay = Layout(pad, raw_bytes - SLACK - pad, r - pad, mis)
    check_layout(lay, raw_ptr, raw_bytes)
    return lay


def check_layout(lay: Layout, raw_ptr: int, raw_bytes: int = RAW_BYTES) -> None:
    assert (raw_ptr + lay.pad) % 16 == lay.mis
    assert (raw_ptr + lay.pad + lay.addr_line) % LINE == 0
    assert MARGIN <= lay.addr_line <= LINE - MARGIN, lay
    assert lay.data_len > MIN_DATA and lay.data_len - lay.addr_line >= MARGIN, lay
    assert lay.pad >= SLACK and lay.pad + lay.data_len + SLACK <= raw_bytes, lay


# ---------------------------------------------------------------- stages
@dataclass
class Desc:
    off: int
    cap: int
    line: int                      # index into Layout.lines
    pkt: cc.Pkt | None = None      # a checksum_cases packet: its expected values are known
    tag: str = ""                  # what the descriptor is there for
    k: int | None = None           # the line lies k bytes into the packet (0 < k < cap: it straddles)
    dead: int = 0                  # cc.DEAD_*


@dataclass
class Stage:
    name: str
    descs: list[Desc]
    extents: list[tuple[int, np.ndarray]]   # (wide offset, bytes): what has to be in the wide buffer
    compact: PacketBatch                    # the same packets in a small buffer
    stream: list[bool]                      # per tile, by cc.tile_streams over the wide descriptors
    meta: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return len(self.descs)

    @property
    def offsets(self) -> np.ndarray:
        return np.array([d.off for d in self.descs], dtype=np.uint64)

    @property
    def caplens(self) -> np.ndarray:
        return np.array([d.cap for d in self.descs], dtype=np.uint32)

    def known(self) -> np.ndarray:
        """The descriptors whose checksum fields the Python reference knows (and the dead ones)."""
        return np.array([i for i, d in enumerate(self.descs) if d.pkt is not None or d.dead], dtype=np.int64)

    def case_batch(self) -> cc.CaseBatch:
        """The known() descriptors as a checksum_cases batch over the compact buffer."""
        idx = self.known()
        exp = np.zeros(len(idx), cc.EXPECT_DTYPE)
        labels = []
        for j, i in enumerate(idx):
            d = self.descs[int(i)]
            if d.dead:
                exp[j]["dead"] = d.dead
            else:
                exp[j] = cc.expect_row(d.pkt, d.off)
            labels.append(f"{d.tag} line{d.line} {d.pkt.family if d.pkt else ''}")
        b = PacketBatch(self.compact.data, self.compact.offsets[idx].copy(), self.compact.caplens[idx].copy())
        return cc.CaseBatch(self.name, b, exp, labels)


def in_bounds(off: int, cap: int, data_len: int) -> bool:
    return off + cap <= data_len  # Python integers: the contract without any wrap


def finish(name: str, descs: list[Desc], data_len: int, bytes_of: dict[int, bytes]) -> Stage:
    """bytes_of: descriptor index -> its bytes (the live descriptors). Builds the extents (placements closer than 4 KiB
    merged, the gaps FILL) and the compact batch (extents 64 B and more apart, each at its wide address mod 16)."""
    assert len(descs) % TILE == 0
    spans = sorted((descs[i].off, b) for i, b in bytes_of.items() if len(b))
    extents: list[tuple[int, bytearray]] = []
    for off, b in spans:
        if extents and off <= extents[-1][0] + len(extents[-1][1]) + 4096:
            s, buf = extents[-1]
            if off + len(b) > s + len(buf):
                buf.extend(bytes([cc.FILL]) * (off + len(b) - s - len(buf)))
            old = bytes(buf[off - s: off - s + len(b)])
            assert all(o in (cc.FILL, n) for o, n in zip(old, b)) or old == b, (name, "packets collide at", off)
            buf[off - s: off - s + len(b)] = b
        else:
            extents.append((off, bytearray(b)))
    starts = [s for s, _ in extents]
    cstart, pos = [], 64
    for s, buf in extents:
        pos += (s - pos) % 16
        cstart.append(pos)
        pos += len(buf) + 64
    cdata = np.full(pos + 64, cc.FILL, np.uint8)
    for c, (_, buf) in zip(cstart, extents):
        cdata[c:c + len(buf)] = np.frombuffer(bytes(buf), np.uint8)
    coffs = np.zeros(len(descs), np.uint64)
    for i, d in enumerate(descs):
        if not in_bounds(d.off, d.cap, data_len):
            assert d.dead == cc.DEAD_BAD_DESC and d.cap >= 1, (name, i)
            coffs[i] = d.off if d.off >= 1 << 63 else len(cdata)  # bad there as well
            continue
        assert d.dead in (0, cc.DEAD_EMPTY, cc.DEAD_OVERSIZE) and (d.cap == 0) == (d.dead == cc.DEAD_EMPTY), (name, i)
        assert (d.cap > 65535) == (d.dead == cc.DEAD_OVERSIZE), (name, i)
        if d.cap == 0:
            coffs[i] = 64
            continue
        e = bisect.bisect_right(starts, d.off) - 1
        assert e >= 0 and d.off + d.cap <= starts[e] + len(extents[e][1]), (name, i)
        coffs[i] = d.off - starts[e] + cstart[e]
    compact = PacketBatch(cdata, coffs, np.array([d.cap for d in descs], np.uint32))
    for i, b in bytes_of.items():
        assert compact.packet(i) == b, (name, i)
    wide = PacketBatch(np.zeros(0, np.uint8), np.array([d.off for d in descs], np.uint64), compact.caplens)
    stream = [_tile_streams(wide, t, data_len) for t in range(len(descs) // TILE)]
    ext = [(s, np.frombuffer(bytes(buf), np.uint8).copy()) for s, buf in extents]
    for s, a in ext:
        assert s >= SLACK and s + len(a) <= data_len
    return Stage(name, descs, ext, compact, stream)


def _tile_streams(wide: PacketBatch, t: int, data_len: int) -> bool:
    """cc.tile_streams over descriptors whose buffer is not there: only its length enters."""
    return cc.tile_streams(SimpleNamespace(offsets=wide.offsets, caplens=wide.caplens, n=wide.n,
                                           data=SimpleNamespace(nbytes=data_len)), t)


def _neighbours(seed: int, count: int) -> list[cc.Pkt]:
    pkts, _ = cc.s1_packets()
    start = (seed * 131) % (len(pkts) - count)
    return list(pkts[start:start + count])


def around(descs: list[Desc], bytes_of: dict[int, bytes], line: int, L: int, centre, k, seed: int, tag: str,
           n_below: int = 31, n_above: int = 32, above_at: int | None = None, order: str = "ascending",
           dead_every: int = 0, data_len: int = 0) -> None:
    """One tile for line L: the centre packet (a cc.Pkt or bytes; None: none) with the line k bytes into it, n_below
    packets packed up to its first byte and n_above packed from its last one (or from above_at)."""
    assert (1 if centre is not None else 0) + n_below + n_above == TILE
    nb = _neighbours(seed, n_below + n_above)
    mine: list[tuple[Desc, bytes]] = []
    if centre is not None:
        data = centre.data if isinstance(centre, cc.Pkt) else centre
        start, end = L - k, L - k + len(data)
        mine.append((Desc(start, len(data), line, centre if isinstance(centre, cc.Pkt) else None, tag, k), data))
    else:
        start = end = L
    pos = start
    below = []
    for p in nb[:n_below]:
        pos -= len(p.data)
        below.append((Desc(pos, len(p.data), line, p, "below"), p.data))
    pos = end if above_at is None else above_at
    above = []
    for p in nb[n_below:]:
        above.append((Desc(pos, len(p.data), line, p, "above"), p.data))
        pos += len(p.data)
    if order == "ascending":
        seq = below[::-1] + mine + above
    else:  # the first live lane is the packet above the line, the others lie below it
        seq = above[:1] + below + mine + above[1:]
    if dead_every:
        for j in range(2, len(seq), dead_every):
            if seq[j][0].k is not None:
                continue
            kind = (cc.DEAD_BAD_DESC, cc.DEAD_EMPTY)[(j // dead_every) % 2]
            d = seq[j][0]
            seq[j] = (Desc(data_len - 8, 64, line, None, "dead", dead=kind), b"") if kind == cc.DEAD_BAD_DESC else \
                (Desc(d.off, 0, line, None, "dead", dead=kind), b"")
    for d, b in seq:
        if b:
            bytes_of[len(descs)] = b
        descs.append(d)


PAYLOAD = 300


def _pkt(family: str, seed: int, **kw) -> cc.Pkt:
    return cc.build(family, np.random.default_rng(seed).bytes(PAYLOAD), **kw)


def straddlers() -> list[tuple[str, object, int]]:
    """(tag, packet, k): the line lies k bytes into the packet."""
    from mutate import crafted, crafted_http

    out: list[tuple[str, object, int]] = []
    seed = 0
    for f in cc.FAMILIES:
        v4, tcp = f.startswith("IPv4"), f.endswith("TCP")
        p = _pkt(f, seed := seed + 1)
        l4, l4h, n = p.l4_off, (20 if tcp else 8), len(p.data)
        out.append((f"ip_addr/{f}", p, 14 + (14 if v4 else 8 + 10)))       # inside the hashed source address
        out.append((f"ip_addr2/{f}", p, 14 + (18 if v4 else 24 + 7)))      # inside the destination address
        out.append((f"l4_ports/{f}", p, l4 + 2))
        # the stored checksum field across the line; half of them do not verify
        bad = _pkt(f, seed := seed + 1, l4_stored=0x1234 if tcp else 0xBEEF) if v4 else p
        out.append((f"l4_csum/{f}", bad, l4 + (17 if tcp else 7)))
        out.append((f"l4_edge/{f}", p, l4 + l4h + 3))                       # 0 < k - l4 < 32: the first chunks of the sum
        out.append((f"l4_edge5/{f}", p, l4 + 5))
        out.append((f"l4_whole/{f}", p, l4 + l4h + 150 + seed % 16))
        out.append((f"l4_tail/{f}", p, n - 3 - seed % 8))
        out.append((f"start_minus1/{f}", p, 1))
        out.append((f"end_plus1/{f}", p, n - 1))
    p = _pkt("IPv4/TCP", 50, ip_stored=0x4321)
    out.append(("eth/IPv4/TCP", p, 7))
    out.append(("eth_type/IPv6/UDP", _pkt("IPv6/UDP", 51), 13))
    for f, k in (("IPv4/TCP", 112), ("IPv6/UDP", 112), ("IPv4/UDP", 136), ("IPv6/TCP", 136), ("IPv4/TCP", 96),
                 ("IPv6/TCP", 128), ("IPv4/UDP", 144)):
        out.append((f"window_gap{k}/{f}", _pkt(f, 60 + k), k))
    out.append(("vlan/IPv4/UDP", _pkt("IPv4/UDP", 70, vlans=2), 14 + 3))
    out.append(("vlan_l4/IPv6/TCP", _pkt("IPv6/TCP", 71, vlans=2, l4_stored=0), 14 + 8 + 40 + 9))
    out.append(("gre/IPv4/TCP", _pkt("IPv4/TCP", 72, gre=True), 14 + 24 + 2))
    out.append(("gre_inner/IPv6/UDP", _pkt("IPv6/UDP", 73, gre=True), 14 + 24 + 4 + 20))
    deep = [b for b in crafted() if len(b) > 200]
    assert len(deep) >= 3
    for j, b in enumerate(deep[:3]):
        out.append((f"deep{j}", b, 150 + 17 * j))
    http = [b for b in crafted_http(200) if len(b) > 260]
    assert len(http) >= 3
    for j, b in enumerate(http[:3]):
        out.append((f"http{j}", b, 170 + 31 * j))
    return out


def stages(lay: Layout) -> list[Stage]:
    out: list[Stage] = []
    lines, dl = lay.lines, lay.data_len

    def stage(name, fn, **meta):
        descs: list[Desc] = []
        bytes_of: dict[int, bytes] = {}
        for li, L in enumerate(lines):
            fn(descs, bytes_of, li, L)
        st = finish(name, descs, dl, bytes_of)
        st.meta.update(meta)
        out.append(st)

    # packet edges on the line: a last byte at L - 1, an empty packet at L and a first byte at L; a first byte at L + 1
    def edges(descs, bytes_of, li, L):
        around(descs, bytes_of, li, L, None, 0, 3, "edge", n_below=31, n_above=33)
        descs[-1] = Desc(L, 0, li, None, "empty_at_line", dead=cc.DEAD_EMPTY)
        del bytes_of[len(descs) - 1]
    stage("edges", edges)
    stage("edge_plus1", lambda d, b, li, L: around(d, b, li, L, None, 0, 4, "edge", n_below=32, n_above=32, above_at=L + 1))
    # one straddling packet per line in a packed ascending tile
    for j, (tag, p, k) in enumerate(straddlers()):
        stage(tag, lambda d, b, li, L, p=p, k=k, tag=tag, j=j: around(d, b, li, L, p, k, 10 + j, tag))
    # tile forms
    c = _pkt("IPv6/TCP", 80)
    stage("permuted", lambda d, b, li, L: around(d, b, li, L, c, 140, 5, "permuted", n_below=62, n_above=1,
                                                      order="above_first"))
    stage("dead", lambda d, b, li, L: around(d, b, li, L, c, 33, 6, "dead_lanes", dead_every=5, data_len=dl))

    def sparse(descs, bytes_of, li, L):
        nb = _neighbours(7 + li, TILE)
        spots = [j for j in range(-SPARSE_REACH, SPARSE_REACH + 1)]
        seq, it = [], iter(nb)
        for j in spots:
            pos = L + j * SPARSE_STRIDE
            if j == 0:
                p = _pkt("IPv4/UDP", 81)
                seq.append((Desc(L - 77, len(p.data), li, p, "sparse", 77), p.data))
                pos = L - 77 + len(p.data)
            for _ in range(8 if j == 0 else 4):
                q = next(it)
                if len(seq) == TILE:
                    break
                seq.append((Desc(pos, len(q.data), li, q, "sparse"), q.data))
                pos += len(q.data)
        assert len(seq) == TILE
        for d, b in seq:
            bytes_of[len(descs)] = b
            descs.append(d)
    stage("sparse", sparse)

    def big1500(descs, bytes_of, li, L):
        rng = np.random.default_rng(1500 + li)
        pk = [cc._sized(rng, j, 1500) for j in range(TILE)]
        assert all(len(p.data) == 1500 for p in pk)
        pos = L - 32 * 1500 - 700
        for j, p in enumerate(pk):
            bytes_of[len(descs)] = p.data
            descs.append(Desc(pos, 1500, li, p, "tile1500", (L - pos) if pos < L < pos + 1500 else None))
            pos += 1500
        # the first descriptor: 64 KiB across the line over the bytes of the packets behind it, one byte too long to parse
        # (select and steer copy it all the same)
        first = len(descs) - TILE
        del bytes_of[first]
        descs[first] = Desc(descs[first + 1].off, 65536, li, None, "oversize_across_line", dead=cc.DEAD_OVERSIZE)
    stage("tile1500", big1500)

    # bad descriptors against a data_len above 2^32, in a tile of live packets next to the offset line (both tiles)
    def bad(descs, bytes_of, li, L):
        first = len(descs)
        around(descs, bytes_of, li, L, c, 60, 8 + li, "bad_tile")
        last = _pkt("IPv4/TCP", 90)  # (both tiles name the same bytes)
        n = len(last.data)
        repl = [(Desc(dl - n, n, li, last, "ends_at_data_len"), last.data),
                (Desc(dl - n + 1, n, li, None, "ends_1_past_data_len", dead=cc.DEAD_BAD_DESC), b""),
                (Desc(2 * LINE + 4096, 64, li, None, "in_bounds_in_32_bits", dead=cc.DEAD_BAD_DESC), b""),
                (Desc(dl + LINE - (1 << 27), 1, li, None, "in_bounds_in_32_bits_b", dead=cc.DEAD_BAD_DESC), b""),
                (Desc(0xFFFFFFFFFFFFFFF0, 64, li, None, "wraps_64_bits", dead=cc.DEAD_BAD_DESC), b""),
                (Desc(dl, 1, li, None, "at_data_len", dead=cc.DEAD_BAD_DESC), b""),
                (Desc(dl, 0, li, None, "empty_at_data_len", dead=cc.DEAD_EMPTY), b"")]
        for j, (d, b) in enumerate(repl):  # replace neighbours well away from the centre packet
            i = first + 2 + 3 * j
            assert descs[i].k is None
            descs[i] = d
            bytes_of.pop(i, None)
            if b:
                bytes_of[i] = b
    stage("bad_desc", bad)
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return out


def straddles(d: Desc, L: int) -> bool:
    return d.off < L < d.off + d.cap


# ---------------------------------------------------------------- outputs past 2^32: one period, repeated
BLOCK_BYTES = MIB
P = 251


@dataclass
class Period:
    block: np.ndarray     # u8[BLOCK_BYTES]
    offsets: np.ndarray   # u64[P]
    caplens: np.ndarray   # u32[P]
    keep: np.ndarray | None     # select: u8[P], about 3/4 kept
    bucket: np.ndarray | None   # steer: u8[P], a few dropped values
    K: int

    def sums(self) -> list[int]:
        """Output bytes per period: of the kept packets, or of each bucket."""
        ln = self.caplens.astype(np.int64)
        if self.keep is not None:
            return [int(ln[self.keep != 0].sum())]
        return [int(ln[self.bucket == b].sum()) for b in range(self.K)]


JUMBOS = (17, 201)


def _period(K: int, seed: int) -> Period:
    """K = 0: select."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2001, P).astype(np.uint32)
    lens[40:47] = 0          # zero-length runs
    lens[130:133] = 0
    lens[-2:] = 0
    lens[JUMBOS[0]], lens[JUMBOS[1]] = 9000, 65535
    keep = bucket = None
    if K == 0:
        keep = (rng.random(P) < 0.75).astype(np.uint8) * np.uint8(0x81)
        keep[list(JUMBOS)] = 1
    else:
        # K = 3: one fat bucket between two thin ones. Its own bytes pass 2^32 (the block byte prefix inside a bucket is
        # relative to the bucket's start), and the last bucket starts past 2^32
        bucket = (rng.choice(3, P, p=(0.02, 0.96, 0.02)) if K == 3 else rng.integers(0, K, P)).astype(np.uint8)
        bucket[rng.random(P) < 0.04] = K
        bucket[rng.random(P) < 0.03] = 255
        bucket[JUMBOS[0]], bucket[JUMBOS[1]] = (1 if K == 3 else 0), 1
        ln = lens.astype(np.int64)
        for b in range(K):  # every bucket's bytes odd: one of its packets a byte longer where they are even
            if int(ln[bucket == b].sum()) % 2 == 0:
                i = next((int(i) for i in np.nonzero(bucket == b)[0] if 1 <= lens[i] < 2000), None)
                if i is not None:  # (else: the next seed)
                    lens[i] += 1
                    ln[i] += 1
    offs = np.array([int(rng.integers(0, BLOCK_BYTES - int(x) + 1)) for x in lens], dtype=np.uint64)
    block = np.random.default_rng(seed + 1).integers(0, 256, BLOCK_BYTES, dtype=np.uint8)
    return Period(block, offs, lens, keep, bucket, K)


@lru_cache(maxsize=None)
def period(K: int) -> Period:
    """The period for select (K = 0: the seed is chosen so that the kept bytes are odd) or for K buckets. Odd sums: every
    repetition lands on a new destination alignment."""
    for seed in range(2000 + K, 4000, 97):
        p = _period(K, seed)
        if all(s % 2 == 1 for s in p.sums()):
            return p
    raise AssertionError("no seed with odd period sums")


def repeats(bytes_per_period: int) -> int:
    """R with R * S >= 2^32 + 2^28."""
    return -(-(LINE + (1 << 28)) // bytes_per_period)
