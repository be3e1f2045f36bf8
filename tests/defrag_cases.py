"""Case generators, models and runners for pcppx_defrag_device / pcppx_defrag_reference (tests/test_defrag.py).

A Case is a source batch, its parse records and pcppx_reasm_info (from the oracle's restatements, possibly crafted
afterwards: info is an input column) and the output's capacities. Three runners produce the same Buffers from it --
brute() (the contract of include/pcppx.h restated as a per-packet Python loop), run_reference()
(pcppx_defrag_reference) and run_device() (pcppx_defrag_device) -- every buffer pre-filled with 0xA5 and
over-allocated, so equality of the whole buffers also shows that nothing beyond the output was touched, and nothing at
all but the totals on overflow.

stream() is a second, independent model: IPReassembly::processPacket + matchOutOfOrderFragments
(Packet++/src/IPReassembly.cpp:281-515, 640-701) restated as a streaming machine keyed by ip_key, with the duplicate
and out-of-order paths; tests/test_defrag.py pins it to the reference's own test vectors and then checks the contract's
reassembled packets against it.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, replace

import numpy as np

import mover_cases as mc
import oracle
from mover_cases import F32, F64, FILL
from pcapplusplus_amd import abi
from pcapplusplus_amd.pcap import PacketBatch, from_packets

BLOCK = 1024  # packets per block of the collect / count / place kernels (pcppx_internal.h kDefragBlockPk)
ML = 6        # max_layers of the cases' records
OPTS = abi.make_opts(0, 8, True, ML)
P_IPV4 = 2
MAX_FRAGS = abi.DEFRAG_MAX_FRAGS
FILL8 = 0xA5


@dataclass
class Case(mc.Case):
    summary: np.ndarray | None = None  # SUMMARY_DTYPE[n]
    layers: np.ndarray | None = None   # LAYER_DTYPE[n, ML]
    info: np.ndarray | None = None     # REASM_DTYPE[n]
    passthrough: bool = True
    max_fragments: int = 0
    use_brief: bool = False
    want_columns: bool = True          # first / frags / disposition (index: want_index)
    src_misalign: int = 0

    def batch(self) -> PacketBatch:
        return PacketBatch(self.data, self.offsets, self.caplens)


@dataclass
class Buffers(mc.Buffers):
    first: np.ndarray | None
    frags: np.ndarray | None
    disposition: np.ndarray | None
    totals: np.ndarray


FIELDS = ("offsets", "caplens", "index", "first", "frags", "disposition", "data")


def alloc(c: Case) -> Buffers:
    col = c.want_columns
    return Buffers(*mc.alloc(c), np.full(c.maxp() + mc.PAD_ENTRIES, F32, np.uint32) if col else None,
                   np.full(c.maxp() + mc.PAD_ENTRIES, FILL8, np.uint8) if col else None,
                   np.full(c.n + mc.PAD_ENTRIES, FILL8, np.uint8) if col else None,
                   np.full(abi.DEFRAG_TOTALS, F64, np.uint64))


# ------------------------------------------------------------------ the contract, one packet at a time
def candidates(c: Case):
    """Per packet: ("bad" | "pass" | "left" | "cand", (ip_off, hdr, len) for a candidate)."""
    out = []
    data_len = c.dlen()
    for i in range(c.n):
        off, cap = int(c.offsets[i]), int(c.caplens[i])
        if off + cap > data_len:
            out.append(("bad", None))
            continue
        st = int(c.info["ip_status"][i])
        if st & 15 != abi.IPR_FRAGMENT:
            out.append(("pass", None))
            continue
        kind, geo = "left", None
        if not st & abi.IPR_F_IPV6:
            for k in range(min(int(c.summary["n_layers"][i]), ML)):
                L = c.layers[i, k]
                if int(L["proto"]) != P_IPV4:
                    continue
                o, h, d = int(L["offset"]), int(L["hdr_len"]), int(L["data_len"])
                if h >= 20 and h <= d and o + d <= cap:
                    kind, geo = "cand", (o, h, d - h)
                break
        out.append((kind, geo))
    return out


def header_checksum(hdr: bytes) -> int:
    s = 0
    for k in range(0, len(hdr), 2):
        s += (hdr[k] << 8) | (hdr[k + 1] if k + 1 < len(hdr) else 0)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def patched(pkt: bytearray, ip_off: int, hdr: int, total: int) -> bytes:
    """The reassembled packet's header fields: total length, no fragment word, the checksum."""
    pkt[ip_off + 2:ip_off + 4] = struct.pack(">H", (hdr + total) & 0xFFFF)  # htobe16 of a uint16_t
    pkt[ip_off + 6:ip_off + 8] = b"\0\0"
    pkt[ip_off + 10:ip_off + 12] = b"\0\0"
    pkt[ip_off + 10:ip_off + 12] = struct.pack(">H", header_checksum(bytes(pkt[ip_off:ip_off + hdr])))
    return bytes(pkt)


def brute(c: Case) -> Buffers:
    """include/pcppx.h's defrag contract restated."""
    out = alloc(c)
    kinds = candidates(c)
    disp = {"bad": abi.DEFRAG_BAD_DESC, "pass": abi.DEFRAG_PASS, "left": abi.DEFRAG_LEFT, "cand": abi.DEFRAG_LEFT}
    d = [disp[k] for k, _ in kinds]
    groups: dict[int, list[int]] = {}
    for i, (k, _) in enumerate(kinds):
        if k == "cand":
            groups.setdefault(int(c.info["ip_key"][i]), []).append(i)
    ncand = sum(len(g) for g in groups.values())
    out.totals[:] = 0
    out.totals[abi.DEFRAG_CANDIDATES] = ncand
    out.totals[abi.DEFRAG_BAD_DESC_N] = d.count(abi.DEFRAG_BAD_DESC)
    if ncand > (c.max_fragments or c.n):
        out.totals[abi.DEFRAG_OVERFLOW] = 1
        return out
    packets = {}  # completing member -> (sorted members, total)
    for g in groups.values():
        g = sorted(g, key=lambda i: (int(c.info["frag_offset"][i]), i))
        if not 2 <= len(g) <= MAX_FRAGS:
            continue
        total, clean = 0, True
        for k, i in enumerate(g):
            ln = kinds[i][1][2]
            last = bool(int(c.info["ip_status"][i]) & abi.IPR_F_LAST)
            clean = clean and ln > 0 and int(c.info["frag_offset"][i]) == total and last == (k == len(g) - 1)
            total += ln
        o0, h0, _ = kinds[g[0]][1]
        if not clean or o0 + h0 + total > abi.MAX_CAPLEN or h0 + total > 65535:
            continue
        for i in g:
            d[i] = abi.DEFRAG_MERGED
        d[max(g)] = abi.DEFRAG_MERGED_LAST
        packets[max(g)] = (g, total)
    rows = []  # (source, first, frags, bytes)
    for i in range(c.n):
        if d[i] == abi.DEFRAG_MERGED_LAST:
            g, total = packets[i]
            o0, h0, l0 = kinds[g[0]][1]
            src = int(c.offsets[g[0]])
            pkt = bytearray(c.data[src:src + o0 + h0 + l0].tobytes())
            for m in g[1:]:
                o, h, ln = kinds[m][1]
                s = int(c.offsets[m]) + o + h
                pkt += c.data[s:s + ln].tobytes()
            assert len(pkt) == o0 + h0 + total
            rows.append((i, g[0], len(g), patched(pkt, o0, h0, total)))
        elif c.passthrough and d[i] in (abi.DEFRAG_PASS, abi.DEFRAG_LEFT):
            s = int(c.offsets[i])
            rows.append((i, i, 0, c.data[s:s + int(c.caplens[i])].tobytes()))
    nbytes = sum(len(r[3]) for r in rows)
    out.totals[:5] = (len(rows), nbytes, len(packets), sum(len(g) for g, _ in packets.values()),
                      d.count(abi.DEFRAG_LEFT))
    if len(rows) > c.maxp() or (not c.index_only and nbytes > c.cap()):
        out.totals[abi.DEFRAG_OVERFLOW] = 1
        return out
    if out.disposition is not None:
        out.disposition[:c.n] = d
    pos = 0
    for j, (i, f, k, pkt) in enumerate(rows):
        out.offsets[j], out.caplens[j] = pos, len(pkt)
        if out.index is not None:
            out.index[j] = i
        if out.first is not None:
            out.first[j], out.frags[j] = f, k
        if not c.index_only:
            out.data[pos:pos + len(pkt)] = np.frombuffer(pkt, np.uint8)
        pos += len(pkt)
    return out


# ------------------------------------------------------------------ the streaming machine
class _Entry:
    def __init__(self):
        self.data = None   # the reassembled packet so far (IPFragmentData::data)
        self.cur = 0       # currentOffset
        self.ooo = []      # out-of-order list: [offset, payload, last]
        self.geo = None    # (ip_off, hdr) of the first fragment
        self.first = None  # its source number


def _match_out_of_order(e: _Entry) -> bool:
    found_last = False
    while not found_last:
        found = False
        k = 0
        while k < len(e.ooo):
            off, payload, last = e.ooo[k]
            if e.cur == off:
                e.data += payload
                e.cur += len(payload)
                if last:
                    found_last = True  # the scan of the list goes on, as in the reference
                del e.ooo[k]
                found = True
            else:
                k += 1
        if not found:
            break
    return found_last


def stream(c: Case, order=None) -> dict[int, tuple[bytes, int]]:
    """processPacket over the candidates in `order` (source numbers; None: source order) from an empty table:
    {position in order: (the packet returned there with REASSEMBLED, the source number of its first fragment)}."""
    kinds = candidates(c)
    table: dict[int, _Entry] = {}
    out = {}
    for at, i in enumerate(range(c.n) if order is None else order):
        kind, geo = kinds[i]
        if kind != "cand":
            continue
        ip_off, hdr, ln = geo
        key = int(c.info["ip_key"][i])
        st = int(c.info["ip_status"][i])
        foff = int(c.info["frag_offset"][i])
        src = int(c.offsets[i])
        payload = c.data[src + ip_off + hdr:src + ip_off + hdr + ln].tobytes()
        e = table.setdefault(key, _Entry())
        got_last = False
        if st & abi.IPR_F_FIRST:
            if e.data is not None:  # duplicated first fragment
                continue
            e.data = bytearray(c.data[src:src + ip_off + hdr + ln].tobytes())
            e.cur, e.geo, e.first = ln, (ip_off, hdr), i
            got_last = _match_out_of_order(e)
        elif e.cur == foff:
            if e.data is None:  # malformed: not the first fragment, but offset 0
                continue
            e.data += payload
            e.cur += ln
            got_last = True if st & abi.IPR_F_LAST else _match_out_of_order(e)
        elif foff > e.cur:
            e.ooo.append([foff, payload, bool(st & abi.IPR_F_LAST)])
            continue
        if got_last:
            out[at] = (patched(e.data, e.geo[0], e.geo[1], e.cur), e.first)
            del table[key]
    return out


# ------------------------------------------------------------------ runners
def _records(c: Case):
    """(abi.Records over host arrays, the arrays to keep alive)."""
    lay = np.ascontiguousarray(c.layers) if c.n else np.zeros((1, ML), abi.LAYER_DTYPE)
    if c.use_brief:
        rec = np.zeros(max(c.n, 1), abi.BRIEF_DTYPE)
        for f in abi.BRIEF_DTYPE.names:
            rec[f][:c.n] = c.summary[f]
        r = abi.Records(None, lay.ctypes.data)
        r.brief = rec.ctypes.data
    else:
        rec = np.ascontiguousarray(c.summary) if c.n else np.zeros(1, abi.SUMMARY_DTYPE)
        r = abi.Records(rec.ctypes.data, lay.ctypes.data)
    return r, (rec, lay)


def _spec(c: Case) -> abi.DefragSpec:
    return abi.make_defrag_spec(c.passthrough, c.max_fragments)


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, 1, 0)
    rec, keep = _records(c)
    info = np.ascontiguousarray(c.info) if c.n else np.zeros(1, abi.REASM_DTYPE)
    opt = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = abi.Defragged(opt(out.data), c.cap(), out.offsets.ctypes.data, out.caplens.ctypes.data, opt(out.index),
                      opt(out.first), opt(out.frags), opt(out.disposition), c.maxp(), 0, out.totals.ctypes.data)
    abi.defrag_reference(b, rec, ML, info.ctypes.data, _spec(c), o)
    del keep
    return out


class DeviceRun(mc.Staged):
    """A case's tensors on the device; launch() queues pcppx_defrag_device on a stream, result() reads the buffers."""

    def __init__(self, c: Case, device: str = "cuda:0", source=None):
        """source: see mover_cases.Staged."""
        host = alloc(c)
        super().__init__(c, host, device, source, c.src_misalign)
        u8 = lambda a: self.up(np.ascontiguousarray(a).view(np.uint8).reshape(-1))  # noqa: E731
        pad = lambda a, dt: a if len(a) else np.zeros(1, dt)  # noqa: E731
        if c.use_brief:
            rec = np.zeros(max(c.n, 1), abi.BRIEF_DTYPE)
            for f in abi.BRIEF_DTYPE.names:
                rec[f][:c.n] = c.summary[f]
            self.summary, self.brief = None, u8(rec)
        else:
            self.summary, self.brief = u8(pad(c.summary, abi.SUMMARY_DTYPE)), None
        self.layers = u8(pad(c.layers.reshape(-1), abi.LAYER_DTYPE))
        self.info = u8(pad(c.info, abi.REASM_DTYPE))
        opt = lambda a, dt: self.up(a.view(dt)) if a is not None else None  # noqa: E731
        self.d_first, self.d_frags = opt(host.first, np.int32), opt(host.frags, np.uint8)
        self.d_disp = opt(host.disposition, np.uint8)
        self.d_tot = self.up(host.totals.view(np.int64))

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.defrag_device(self.data, self.offsets, self.caplens, c.n, 1, self.layers, ML, self.info, _spec(c),
                             self.d_off, self.d_cap, self.d_tot, c.maxp(), self.d_data, c.cap(), self.d_idx,
                             self.d_first, self.d_frags, self.d_disp, stream, data_len=self.data_len,
                             summary=self.summary, brief=self.brief)

    def result(self) -> Buffers:
        return Buffers(*self.common(), self.down(self.d_first, np.uint32), self.down(self.d_frags, np.uint8),
                       self.down(self.d_disp, np.uint8), self.down(self.d_tot, np.uint64))


def run_device(engine, c: Case, device: str = "cuda:0", source=None) -> Buffers:
    import torch

    run = DeviceRun(c, device, source)
    run.launch(engine, torch.cuda.current_stream(device).cuda_stream)
    return run.result()


def assert_same(got: Buffers, want: Buffers, what: str) -> None:
    mc.assert_same(got, want, what, FIELDS)


def assert_untouched(got: Buffers, what: str) -> None:
    """The all-or-nothing rule: every column and the data still hold the fill, every byte of them."""
    for f, fill in (("data", FILL), ("offsets", F64), ("caplens", F32), ("index", F32), ("first", F32),
                    ("frags", FILL8), ("disposition", FILL8)):
        g = getattr(got, f)
        assert g is None or bool((g == fill).all()), (what, f)


def reassembled(got: Buffers) -> list[tuple[int, int, bytes]]:
    """(source number, first, bytes) of every reassembled packet of a run's output."""
    n = int(got.totals[abi.DEFRAG_OUT_PACKETS])
    out = []
    for j in range(n):
        if got.frags[j]:
            o, ln = int(got.offsets[j]), int(got.caplens[j])
            out.append((int(got.index[j]), int(got.first[j]), got.data[o:o + ln].tobytes()))
    return out


# ------------------------------------------------------------------ packets
def eth(vlan: int | None = None, ethertype: int = 0x0800) -> bytes:
    mac = bytes.fromhex("020000000001") + bytes.fromhex("020000000002")
    if vlan is None:
        return mac + struct.pack(">H", ethertype)
    return mac + struct.pack(">HHH", 0x8100, vlan, ethertype)


def ipv4(src: int, dst: int, ipid: int, payload: bytes, proto: int = 17, foff: int = 0, mf: bool = False,
         df: bool = False, options: bytes = b"", total: int | None = None) -> bytes:
    """An IPv4 header (+ options, a multiple of 4 bytes) and payload; foff in bytes."""
    assert foff % 8 == 0 and len(options) % 4 == 0
    ihl = 5 + len(options) // 4
    word = (foff // 8) | (0x2000 if mf else 0) | (0x4000 if df else 0)
    tot = ihl * 4 + len(payload) if total is None else total
    h = bytearray(struct.pack(">BBHHHBBHII", 0x40 | ihl, 0, tot, ipid, word, 64, proto, 0, src, dst) + options)
    h[10:12] = struct.pack(">H", header_checksum(bytes(h)))
    return bytes(h) + payload


def udp_datagram(rng, size: int, sport: int = 4000, dport: int = 5000) -> bytes:
    """A UDP header + size - 8 payload bytes (checksum 0: not computed)."""
    return struct.pack(">HHHH", sport, dport, size, 0) + rng.integers(0, 256, size - 8, dtype=np.uint8).tobytes()


def split(datagram: bytes, sizes: list[int]) -> list[tuple[int, bytes, bool]]:
    """(offset, piece, more fragments) per fragment: pieces of the given sizes (all but the last a multiple of 8)."""
    assert sum(sizes) == len(datagram) and all(s % 8 == 0 for s in sizes[:-1])
    out, at = [], 0
    for k, s in enumerate(sizes):
        out.append((at, datagram[at:at + s], k + 1 < len(sizes)))
        at += s
    return out


def group(rng, ipid: int, sizes: list[int], src: int = 0x0A000001, dst: int = 0x0A000002, vlan: int | None = None,
          options: bytes = b"", trailer: bytes = b"", df_first: bool = False, l2: bytes | None = None) -> list[bytes]:
    """The fragments of one UDP datagram, in offset order; the first may carry a trailer and DF."""
    l2 = eth(vlan) if l2 is None else l2
    pk = []
    for off, piece, more in split(udp_datagram(rng, sum(sizes)), sizes):
        p = l2 + ipv4(src, dst, ipid, piece, foff=off, mf=more, options=options, df=df_first and off == 0)
        pk.append(p + (trailer if off == 0 else b""))
    return pk


def filler(rng, k: int) -> bytes:
    """A small unfragmented UDP packet."""
    return eth() + ipv4(0x0A010000 + k % 251, 0x0A020000 + k % 241, k & 0xFFFF, udp_datagram(rng, 8 + k % 17))


def ipv6_fragment(rng, k: int) -> bytes:
    """An IPv6 packet with a fragment header (offset 0, more fragments)."""
    payload = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
    frag = struct.pack(">BBHI", 17, 0, 1, 0x1000 + k)
    v6 = struct.pack(">IHBB", 0x60000000, len(frag) + len(payload), 44, 64) + bytes(15) + b"\1" + bytes(15) + b"\2"
    return eth(ethertype=0x86DD) + v6 + frag + payload


def gre_group(rng, ipid: int, sizes: list[int]) -> list[bytes]:
    """IPv4-in-GRE, the outer IPv4 packet fragmented: the outer header is the first IPv4 layer, the one patched."""
    inner = ipv4(0xC0A80001, 0xC0A80002, 7, udp_datagram(rng, sum(sizes) - 24))
    gre = struct.pack(">HH", 0, 0x0800) + inner
    assert len(gre) == sum(sizes)
    return [eth() + ipv4(0x0A000009, 0x0A00000A, ipid, piece, proto=47, foff=off, mf=more)
            for off, piece, more in split(gre, sizes)]


def make(name: str, packets: list[bytes], **kw) -> Case:
    """A case over the packets back to back: records and info from the oracle's restatements."""
    b = from_packets(packets) if packets else PacketBatch(np.zeros(1, np.uint8), np.zeros(0, np.uint64),
                                                          np.zeros(0, np.uint32))
    summary, layers = oracle.oracle_parse(b, OPTS)
    info = oracle.oracle_reasm(b, summary, layers)
    data = b.data[:int(b.caplens.sum())] if packets else np.zeros(0, np.uint8)
    return Case(name, data, b.offsets, b.caplens, summary=summary, layers=layers, info=info.copy(), **kw)


def permuted(c: Case, perm) -> Case:
    """The same packets in another order: descriptors, records and info move together."""
    perm = np.asarray(perm)
    return replace(c, offsets=c.offsets[perm], caplens=c.caplens[perm], summary=c.summary[perm],
                   layers=c.layers[perm], info=c.info[perm])


def spread(rng, groups: list[list[bytes]], n: int, places: list[list[int]] | None = None,
           extra: dict[int, bytes] | None = None) -> list[bytes]:
    """n packets: the groups' fragments at the given places (or at random ones, each group in its list's order), the
    packets of `extra` at theirs, fillers everywhere else."""
    out: list[bytes | None] = [None] * n
    for k, p in (extra or {}).items():
        out[k] = p
    if places is None:
        free = [k for k in range(n) if out[k] is None]
        take = np.sort(rng.choice(len(free), sum(len(g) for g in groups), replace=False))
        order = rng.permutation(np.repeat(np.arange(len(groups)), [len(g) for g in groups]))
        nxt = [0] * len(groups)
        for t, gi in zip(take, order):
            out[free[int(t)]] = groups[int(gi)][nxt[int(gi)]]
            nxt[int(gi)] += 1
    else:
        for g, pl in zip(groups, places):
            assert len(g) == len(pl)
            for p, k in zip(g, pl):
                assert out[k] is None
                out[k] = p
    return [p if p is not None else filler(rng, k) for k, p in enumerate(out)]


def sizes_for(k: int, rng, lo: int = 8, hi: int = 24) -> list[int]:
    """k fragment sizes: multiples of 8 in lo..hi, the last one any length in lo..hi."""
    s = [int(x) * 8 for x in rng.integers(lo // 8, hi // 8 + 1, k)]
    s[-1] = int(rng.integers(lo, hi + 1))
    return s


def output_totals(c: Case):
    t = brute(replace(c, data_cap=None, max_packets=None, max_fragments=0, index_only=True)).totals
    return int(t[abi.DEFRAG_OUT_PACKETS]), int(t[abi.DEFRAG_OUT_BYTES]), int(t[abi.DEFRAG_CANDIDATES])


# ------------------------------------------------------------------ the families
CLEAN = []    # names of the cases all of whose IPv4 fragment groups are clean: every one must be reassembled
UNCLEAN = []  # names of the cases whose crafted group must stay LEFT
BIG_N = 66 * BLOCK + 7  # more block sums than one step of the base scan takes


def _clean(c: Case) -> Case:
    CLEAN.append(c.name)
    return c


def _unclean(c: Case) -> Case:
    UNCLEAN.append(c.name)
    return c


def cases() -> list[Case]:
    CLEAN.clear()
    UNCLEAN.clear()
    out: list[Case] = []
    rng = np.random.default_rng(2024)
    # group sizes, in order, reversed and shuffled, alone in the batch
    for k in (2, 3, 63, 64):
        g = group(rng, 0x100 + k, sizes_for(k, rng))
        out.append(_clean(make(f"g{k}_in_order", g)))
        out.append(_clean(make(f"g{k}_reversed", g[::-1])))
        out.append(_clean(make(f"g{k}_shuffled", [g[int(j)] for j in rng.permutation(k)])))
    g = group(rng, 0x165, sizes_for(65, rng))
    out.append(_unclean(make("g65_too_many", g)))
    out.append(_unclean(make("g65_too_many_shuffled", [g[int(j)] for j in rng.permutation(65)], passthrough=False)))
    # members of one group in different tiles and blocks, at both sides of the block size; many groups among fillers
    g3 = group(rng, 0x201, [16, 24, 11])
    g4 = group(rng, 0x202, [8, 8, 8, 9], vlan=5)
    for n in (BLOCK - 1, BLOCK, BLOCK + 1):
        places = [[0, n // 2, n + 70], [n + 71, 63, 64, n - 1]]  # the completing members in the second block
        out.append(_clean(make(f"blocks_n{n}", spread(rng, [g3, g4], n + 72, places))))
    places = [[BLOCK, BLOCK - 1, 5], [2 * BLOCK + 3, BLOCK + 64, BLOCK + 63, 0]]  # the first member last, blocks apart
    out.append(_clean(make("blocks_first_last", spread(rng, [g3, g4], 2 * BLOCK + 4, places))))
    many = [group(rng, 0x1000 + j, sizes_for(2 + j % 5, rng), src=0x0A000100 + j) for j in range(150)]
    out.append(_clean(make("many_groups", spread(rng, many, 3 * BLOCK + 17))))
    out.append(_clean(make("many_groups_only", spread(rng, many, 3 * BLOCK + 17), passthrough=False)))
    out.append(_clean(replace(make("many_groups_brief", spread(rng, many[:40], BLOCK + 300)), use_brief=True,
                              out_misalign=5, src_misalign=11)))
    big = [group(rng, 0x3000 + j, sizes_for(2 + j % 3, rng), src=0x0A100000 + j) for j in range(300)]
    out.append(_clean(make("big", spread(rng, big, BIG_N))))
    # the unclean families: one crafted group, and a clean one beside it that must still be reassembled
    ok = group(rng, 0x400, [16, 16, 9])

    def crafted(name: str, frs: list[bytes], **kw) -> None:
        out.append(_unclean(make(name, spread(rng, [frs, ok], len(frs) + len(ok) + 9), **kw)))

    d = udp_datagram(rng, 48)
    fr = lambda off, piece, more, ipid: eth() + ipv4(0x0A000001, 0x0A000002, ipid, piece, foff=off, mf=more)  # noqa
    crafted("gap", [fr(0, d[:16], True, 0x410), fr(24, d[24:], False, 0x410)])
    crafted("overlap", [fr(0, d[:24], True, 0x411), fr(16, d[16:], False, 0x411)])
    crafted("duplicate", [fr(0, d[:16], True, 0x412), fr(16, d[16:32], True, 0x412), fr(16, d[16:32], True, 0x412),
                          fr(32, d[32:], False, 0x412)])
    two = [fr(0, d[:16], True, 0x413), fr(16, d[16:], False, 0x413)]
    crafted("two_copies", two + two)
    crafted("last_in_the_middle", [fr(0, d[:16], True, 0x414), fr(16, d[16:32], False, 0x414),
                                   fr(32, d[32:], False, 0x414)])
    crafted("no_last", [fr(0, d[:16], True, 0x415), fr(16, d[16:32], True, 0x415), fr(32, d[32:], True, 0x415)])
    crafted("zero_length", [fr(0, d[:16], True, 0x416), fr(16, b"", True, 0x416), fr(16, d[16:], False, 0x416)])
    crafted("no_first", [fr(16, d[16:32], True, 0x417), fr(32, d[32:], False, 0x417)])
    crafted("single", [fr(0, d[:16], True, 0x418)])
    # totals at the two size bounds: hdr + total <= 65535, and ip_off + hdr + total <= PCPPX_MAX_CAPLEN (with a VLAN
    # tag ip_off is 18: the caplen bound is the tighter one)
    for name, total, vlan, good in (("total_65515", 65515, None, False), ("total_65516", 65516, None, False),
                                    ("total_65501", 65501, None, True), ("total_65502", 65502, None, False),
                                    ("total_vlan_65497", 65497, 5, True), ("total_vlan_65498", 65498, 5, False)):
        sz = [total // 2 // 8 * 8]
        sz.append(total - sz[0])
        c = make(name, spread(rng, [group(rng, 0x420, sz, vlan=vlan)], 5))
        out.append(_clean(c) if good else _unclean(c))
    # options, a trailer behind the first fragment, DF on it, VLAN, IPv4 in GRE
    opt = bytes([7, 7, 4, 0, 0, 0, 0, 0])  # record route, one empty slot, end of list padding
    out.append(_clean(make("options", spread(rng, [group(rng, 0x430, [16, 8, 13], options=opt)], 9))))
    out.append(_clean(make("trailer", spread(rng, [group(rng, 0x431, [8, 24, 3], trailer=bytes(range(1, 13)))], 9))))
    out.append(_clean(make("df_first_last", spread(rng, [group(rng, 0x432, [16, 16, 5], vlan=9, df_first=True,
                                                           trailer=b"\0" * 6)[::-1]], 9))))
    out.append(_clean(make("vlan", spread(rng, [group(rng, 0x433, [24, 8, 8, 1], vlan=100)], 11))))
    out.append(_clean(make("gre", spread(rng, [gre_group(rng, 0x434, [16, 24, 12])], 9))))
    # crafted info: unrelated packets under one key merge as in the reference; keys congruent modulo every table size
    # up to 1024 and key 0 (key 0 beside other keys is what that case reaches: the home slot comes from the high bits of
    # key * 0x9E3779B1, so congruent keys land on scattered slots like any others; the probe chains, wraps and races are
    # aimed at by tests/table_cases.py); the FRAGMENT status on a packet without an IPv4 layer
    a, b = group(rng, 0x440, [16, 7], src=0x0A000011), group(rng, 0x441, [16, 16, 3], src=0x0A000012)
    c = make("same_key_two_groups", spread(rng, [a, b], 12))  # two first fragments under one key: not a tiling
    c.info["ip_key"][c.info["ip_status"] & 15 == abi.IPR_FRAGMENT] = 0xDEADBEEF
    out.append(_unclean(c))
    x, y = group(rng, 0x442, [16, 16, 7], src=0x0A000013), group(rng, 0x443, [16, 16, 7], src=0x0A000014)
    c = make("same_key_mixed_tiling", spread(rng, [[x[0], y[1], x[2]]], 8))  # one tiling out of two datagrams
    c.info["ip_key"][c.info["ip_status"] & 15 == abi.IPR_FRAGMENT] = 7
    out.append(_clean(c))
    gs = [group(rng, 0x500 + j, sizes_for(2 + j % 3, rng), src=0x0A000200 + j) for j in range(40)]
    c = make("keys_congruent", spread(rng, gs, 200))
    keys = {int(k): j for j, k in enumerate(np.unique(c.info["ip_key"][c.info["ip_status"] & 15 == abi.IPR_FRAGMENT]))}
    for i in range(c.n):
        if int(c.info["ip_status"][i]) & 15 == abi.IPR_FRAGMENT:
            j = keys[int(c.info["ip_key"][i])]
            c.info["ip_key"][i] = 5 + j * 1024 if j else 0  # one residue modulo every table size up to 1024 (not one
            # home slot: see above); key 0
    out.append(_clean(c))
    c = make("fragment_status_without_ipv4", spread(rng, [ok], 10, extra={3: eth(ethertype=0x0806) + bytes(28)}))
    c.info["ip_status"][3] = abi.IPR_FRAGMENT | abi.IPR_F_FIRST
    c.info["ip_key"][3] = c.info["ip_key"][c.info["ip_status"] & 15 == abi.IPR_FRAGMENT][-1]
    out.append(_clean(c))
    # IPv6 fragments, HOST packets and bad descriptors mixed in
    c = make("mixed", spread(rng, many[:12], 300, extra={7: ipv6_fragment(rng, 1), 99: ipv6_fragment(rng, 2),
                                                           150: eth(ethertype=0x8864) + bytes(30)}))
    assert int(c.info["ip_status"][7]) == abi.IPR_FRAGMENT | abi.IPR_F_IPV6 | abi.IPR_F_FIRST
    assert int(c.info["ip_status"][150]) & 15 == abi.IPR_HOST
    out.append(_clean(c))
    for pt in (True, False):
        c = mc.with_bad_descriptors(make(f"bad_desc_pt{int(pt)}", spread(rng, many[:30], 700), passthrough=pt))
        out.append(c)  # a bad descriptor may take a member away: the groups are whatever the contract says
    c = make("shuffled_descriptors", spread(rng, many[:20], 400))
    perm = rng.permutation(c.n)
    out.append(_clean(permuted(c, perm)))  # descriptors in another order than the bytes
    # capacities: exact and one short; index-only; no optional columns
    base = make("cap", spread(rng, many[:25], 500))
    op, ob, nc = output_totals(base)
    for nm, kw in (("cap_exact", dict(data_cap=ob, max_packets=op, max_fragments=nc)), ("cap_short1", dict(data_cap=ob - 1)),
                   ("maxp_short1", dict(max_packets=op - 1)), ("maxf_short1", dict(max_fragments=nc - 1)),
                   ("maxf_1", dict(max_fragments=1)), ("cap_zero", dict(data_cap=0)),
                   ("index_only", dict(index_only=True)), ("index_only_cap_ignored", dict(index_only=True, data_cap=3)),
                   ("index_only_maxp_short1", dict(index_only=True, max_packets=op - 1)),
                   ("no_columns", dict(want_index=False, want_columns=False)),
                   ("only_reassembled", dict(passthrough=False)),
                   ("only_reassembled_exact", dict(passthrough=False, max_packets=25)),
                   ("only_reassembled_short1", dict(passthrough=False, max_packets=24))):
        out.append(replace(base, name=nm, **kw))
    # n = 0, n = 1, no candidates at all
    out.append(make("n0", []))
    out.append(make("n1_fragment", [ok[0]]))
    out.append(make("n1_plain", [filler(rng, 1)]))
    out.append(make("no_candidates", [filler(rng, k) for k in range(BLOCK + 100)]))
    out.append(make("no_candidates_only", [filler(rng, k) for k in range(130)], passthrough=False))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


OVERFLOWING = ("cap_short1", "maxp_short1", "maxf_short1", "maxf_1", "cap_zero", "index_only_maxp_short1",
               "only_reassembled_short1")
