"""Case generators, the model and runners for pcppx_frag_device / pcppx_frag_reference (tests/test_frag.py).

A Case is a source batch, its parse records (from the oracle's restatement, possibly crafted afterwards: the records
are an input), the fragmenting rule and the output's capacities. Three runners produce the same Buffers from it --
brute() (the frag contract of include/pcppx.h restated as a per-packet Python loop), run_reference()
(pcppx_frag_reference) and run_device() (pcppx_frag_device) -- every buffer pre-filled with 0xA5 and over-allocated, so
equality of the whole buffers also shows that nothing beyond the output was touched, and nothing at all but the totals
on overflow.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, replace

import numpy as np

import defrag_cases as dc
import mover_cases as mc
import oracle
from mover_cases import F32, F64, FILL
from pcapplusplus_amd import abi
from pcapplusplus_amd.pcap import PacketBatch, from_packets

BLOCK = 1024  # source packets per block of the plan / emit / patch kernels (pcppx_internal.h kFragBlockPk)
ML = dc.ML
OPTS = dc.OPTS
P_IPV4 = 2
FILL8, F16 = 0xA5, 0xA5A5
ETH, RAW, SLL = abi.LINKTYPE_ETHERNET, abi.LINKTYPE_RAW, abi.LINKTYPE_LINUX_SLL


@dataclass
class Case(mc.Case):
    summary: np.ndarray | None = None  # SUMMARY_DTYPE[n]
    layers: np.ndarray | None = None   # LAYER_DTYPE[n, ML]
    linktype: int = ETH
    frag_size: int = 0
    mtu: int = 0
    keep: np.ndarray | None = None     # u8[n]; None: every packet
    copy_rest: bool = True
    honor_df: bool = False
    use_brief: bool = False
    want_columns: bool = True          # frag_no / counts / disposition (index: want_index)
    src_misalign: int = 0

    def batch(self) -> PacketBatch:
        return PacketBatch(self.data, self.offsets, self.caplens, self.linktype)

    def cap(self) -> int:  # None: exactly what the output needs
        return needs(self)[1] if self.data_cap is None else self.data_cap

    def maxp(self) -> int:
        return needs(self)[0] if self.max_packets is None else self.max_packets


@dataclass
class Buffers(mc.Buffers):
    frag_no: np.ndarray | None
    counts: np.ndarray | None
    disposition: np.ndarray | None
    totals: np.ndarray


FIELDS = ("offsets", "caplens", "index", "frag_no", "counts", "disposition", "data")


def alloc(c: Case) -> Buffers:
    col, mp = c.want_columns, c.maxp()
    return Buffers(None if c.index_only else np.full(c.cap() + mc.PAD_BYTES, FILL, np.uint8),
                   np.full(mp + mc.PAD_ENTRIES, F64, np.uint64), np.full(mp + mc.PAD_ENTRIES, F32, np.uint32),
                   np.full(mp + mc.PAD_ENTRIES, F32, np.uint32) if c.want_index else None,
                   np.full(mp + mc.PAD_ENTRIES, F16, np.uint16) if col else None,
                   np.full(c.n + mc.PAD_ENTRIES, F16, np.uint16) if col else None,
                   np.full(c.n + mc.PAD_ENTRIES, FILL8, np.uint8) if col else None,
                   np.full(abi.FRAG_TOTALS, F64, np.uint64))


# ------------------------------------------------------------------ the contract, one packet at a time
def ipv4_layer(c: Case, i: int, cap: int):
    """(ip_off, hdr, pay) of packet i's IPv4 layer as the contract defines it, or None."""
    for k in range(min(int(c.summary["n_layers"][i]), ML)):
        L = c.layers[i, k]
        if int(L["proto"]) != P_IPV4:
            continue
        o, h, d = int(L["offset"]), int(L["hdr_len"]), int(L["data_len"])
        return (o, h, d - h) if 20 <= h <= 60 and h <= d and o + d <= cap else None  # the first one decides
    return None


def plan(c: Case):
    """Per source packet: (disposition, (ip_off, hdr, pay, fs) for a SPLIT packet)."""
    out = []
    data_len = c.dlen()
    for i in range(c.n):
        off, cap = int(c.offsets[i]), int(c.caplens[i])
        if off + cap > data_len:  # Python integers: no wrap
            out.append((abi.FRAG_BAD_DESC, None))
            continue
        if c.keep is not None and int(c.keep[i]) == 0:
            out.append((abi.FRAG_UNSELECTED, None))
            continue
        geo = ipv4_layer(c, i, cap)
        if geo is None:
            out.append((abi.FRAG_NOT_V4, None))
            continue
        o, h, pay = geo
        word = (int(c.data[off + o + 6]) << 8) | int(c.data[off + o + 7])
        fs = c.frag_size if c.frag_size else (c.mtu - h) & ~7
        if word & 0x3FFF:
            d = abi.FRAG_ALREADY
        elif (pay <= fs) if c.frag_size else (h + pay <= c.mtu):
            d = abi.FRAG_FITS
        elif c.honor_df and word & 0x4000:
            d = abi.FRAG_DF
        else:
            d = abi.FRAG_SPLIT
        out.append((d, (o, h, pay, fs)))
    return out


def fragment_bytes(src: bytes, o: int, h: int, pay: int, fs: int, j: int, count: int) -> bytes:
    piece = src[o + h + j * fs:o + h + min((j + 1) * fs, pay)]
    pkt = bytearray(src[:o + h] + piece)
    pkt[o + 2:o + 4] = struct.pack(">H", h + len(piece))
    pkt[o + 6:o + 8] = struct.pack(">H", (j * fs // 8) | (0x2000 if j < count - 1 else 0))
    pkt[o + 10:o + 12] = b"\0\0"
    pkt[o + 10:o + 12] = struct.pack(">H", dc.header_checksum(bytes(pkt[o:o + h])))
    return bytes(pkt)


def rows_of(c: Case, plans=None):
    """The output packets in order: (source, fragment number, bytes); and the per-source counts."""
    plans = plan(c) if plans is None else plans
    rows, counts = [], []
    for i, (d, geo) in enumerate(plans):
        before = len(rows)
        if d == abi.FRAG_SPLIT:
            o, h, pay, fs = geo
            off = int(c.offsets[i])
            src = c.data[off:off + int(c.caplens[i])].tobytes()
            count = -(-pay // fs)
            rows += [(i, j, fragment_bytes(src, o, h, pay, fs, j, count)) for j in range(count)]
        elif d != abi.FRAG_BAD_DESC and c.copy_rest:
            off = int(c.offsets[i])
            rows.append((i, 0, c.data[off:off + int(c.caplens[i])].tobytes()))
        counts.append(len(rows) - before)
    return rows, counts


_NEEDS: dict[int, tuple] = {}


def needs(c: Case) -> tuple[int, int]:
    """(output packets, output bytes) of the case's rule over its batch, whatever its capacities."""
    key = (id(c.data), id(c.offsets), id(c.caplens), id(c.layers), id(c.summary), id(c.keep), c.frag_size, c.mtu,
           c.copy_rest, c.honor_df, c.data_len)
    if key not in _NEEDS:
        rows, _ = rows_of(c)
        _NEEDS[key] = (len(rows), sum(len(r[2]) for r in rows), c)  # c kept alive: the ids stay its own
    return _NEEDS[key][:2]


def brute(c: Case) -> Buffers:
    """include/pcppx.h's frag contract restated."""
    out = alloc(c)
    plans = plan(c)
    rows, counts = rows_of(c, plans)
    disp = [d for d, _ in plans]
    nbytes = sum(len(r[2]) for r in rows)
    frags = sum(k for k, d in zip(counts, disp) if d == abi.FRAG_SPLIT)
    over = len(rows) > c.maxp() or (not c.index_only and nbytes > c.cap())
    out.totals[:] = (len(rows), nbytes, disp.count(abi.FRAG_SPLIT), frags, len(rows) - frags,
                     disp.count(abi.FRAG_FITS), disp.count(abi.FRAG_BAD_DESC), 1 if over else 0)
    if over:
        return out
    if out.disposition is not None:
        out.disposition[:c.n] = disp
        out.counts[:c.n] = counts
    pos = 0
    for r, (i, j, pkt) in enumerate(rows):
        out.offsets[r], out.caplens[r] = pos, len(pkt)
        if out.index is not None:
            out.index[r] = i
        if out.frag_no is not None:
            out.frag_no[r] = j
        if not c.index_only:
            out.data[pos:pos + len(pkt)] = np.frombuffer(pkt, np.uint8)
        pos += len(pkt)
    return out


# ------------------------------------------------------------------ runners
def spec_of(c: Case, keep_addr) -> abi.FragSpec:
    return abi.make_frag_spec(c.frag_size, c.mtu, keep_addr, c.copy_rest, c.honor_df)


def host_records(c: Case):
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


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, c.linktype, 0)
    rec, alive = host_records(c)
    keep = None if c.keep is None else np.ascontiguousarray(c.keep if c.n else np.zeros(1, np.uint8))
    opt = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = abi.Fragmented(opt(out.data), c.cap(), out.offsets.ctypes.data, out.caplens.ctypes.data, opt(out.index),
                       opt(out.frag_no), opt(out.counts), opt(out.disposition), c.maxp(), 0, out.totals.ctypes.data)
    abi.frag_reference(b, rec, ML, spec_of(c, opt(keep)), o)
    del alive
    return out


class DeviceRun(mc.Staged):
    """A case's tensors on the device; launch() queues pcppx_frag_device on a stream, result() reads the buffers."""

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
        self.keep = None if c.keep is None else self.up(pad(np.ascontiguousarray(c.keep), np.uint8))
        opt = lambda a, dt: self.up(a.view(dt)) if a is not None else None  # noqa: E731
        self.d_no, self.d_cnt = opt(host.frag_no, np.int16), opt(host.counts, np.int16)
        self.d_disp = opt(host.disposition, np.uint8)
        self.d_tot = self.up(host.totals.view(np.int64))

    def launch(self, engine, stream: int) -> None:
        c = self.c
        spec = spec_of(c, None if self.keep is None else abi.ptr(self.keep))
        engine.frag_device(self.data, self.offsets, self.caplens, c.n, c.linktype, self.layers, ML, spec, self.d_off,
                           self.d_cap, self.d_tot, c.maxp(), self.d_data, c.cap(), self.d_idx, self.d_no, self.d_cnt,
                           self.d_disp, stream, data_len=self.data_len, summary=self.summary, brief=self.brief)

    def result(self) -> Buffers:
        return Buffers(*self.common(), self.down(self.d_no, np.uint16), self.down(self.d_cnt, np.uint16),
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
    for f, fill in (("data", FILL), ("offsets", F64), ("caplens", F32), ("index", F32), ("frag_no", F16),
                    ("counts", F16), ("disposition", FILL8)):
        g = getattr(got, f)
        assert g is None or bool((g == fill).all()), (what, f)


def output_batch(got: Buffers, linktype: int = ETH) -> PacketBatch:
    """The output of a run that did not overflow, as a batch."""
    w, wb = int(got.totals[abi.FRAG_OUT_PACKETS]), int(got.totals[abi.FRAG_OUT_BYTES])
    return PacketBatch(np.concatenate([got.data[:wb], np.zeros(1, np.uint8)]), got.offsets[:w].copy(),
                       got.caplens[:w].copy(), linktype)


# ------------------------------------------------------------------ packets
def l2(ip_off: int) -> tuple[bytes, int]:
    """(the link layer in front of an IPv4 header at ip_off, the batch's link type)."""
    if ip_off == 0:
        return b"", RAW
    if ip_off == 16:  # Linux cooked capture: packet type, ARPHRD_ETHER, address length, address, protocol
        return struct.pack(">HHH8sH", 0, 1, 6, bytes.fromhex("0200000000010000"), 0x0800), SLL
    mac = bytes.fromhex("020000000001") + bytes.fromhex("020000000002")
    tags = {14: b"", 18: struct.pack(">HH", 0x8100, 5), 22: struct.pack(">HHHH", 0x88A8, 7, 0x8100, 5)}[ip_off]
    return mac + tags + struct.pack(">H", 0x0800), ETH


def options(hdr: int) -> bytes:
    """IPv4 options that fill a header of hdr bytes: no-operations and an end of list."""
    return b"" if hdr == 20 else b"\x01" * (hdr - 21) + b"\x00"


def v4(rng, k: int, pay: int, ip_off: int = 14, hdr: int = 20, df: bool = False, foff: int = 0, mf: bool = False,
       tcp: bool = False, trailer: bytes = b"", cut: int = 0) -> bytes:
    """An IPv4 packet with `pay` bytes of IP payload (UDP where 8 bytes fit and it is no later fragment); the last
    `cut` bytes not captured."""
    if foff or pay < 8:
        l4 = rng.integers(0, 256, pay, dtype=np.uint8).tobytes()
    elif tcp and pay >= 20:
        l4 = struct.pack(">HHIIBBHHH", 1024 + k % 999, 80, k, 0, 0x50, 0x10, 512, 0, 0) + \
            rng.integers(0, 256, pay - 20, dtype=np.uint8).tobytes()
    else:
        l4 = dc.udp_datagram(rng, pay, 1024 + k % 50, 2000 + k % 7)
    p = l2(ip_off)[0] + dc.ipv4(0x0A000000 + k % 97, 0x0B000000 + k // 97, k & 0xFFFF, l4, proto=6 if tcp else 17,
                                foff=foff, mf=mf, df=df, options=options(hdr)) + trailer
    return p[:len(p) - cut] if cut else p


def make(name: str, packets: list[bytes], linktype: int = ETH, **kw) -> Case:
    """A case over the packets back to back: records from the oracle's restatement."""
    if not packets:
        return Case(name, np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                    summary=np.zeros(0, abi.SUMMARY_DTYPE), layers=np.zeros((0, ML), abi.LAYER_DTYPE), **kw)
    b = from_packets(packets, linktype)
    return over(name, b.data[:int(b.caplens.sum())], b.offsets, b.caplens, linktype, **kw)


def over(name: str, data: np.ndarray, offsets: np.ndarray, caplens: np.ndarray, linktype: int = ETH, **kw) -> Case:
    """A case over any descriptors of `data` (in bounds): the records are the oracle's parse of those descriptors."""
    padded = np.concatenate([data, np.zeros(1, np.uint8)])
    summary, layers = oracle.oracle_parse(PacketBatch(padded, offsets, caplens, linktype), OPTS)
    return Case(name, data, offsets, caplens, summary=summary, layers=layers.copy(), linktype=linktype, **kw)


def permuted(c: Case, perm) -> Case:
    """The same packets in another order: descriptors, records and the keep column move together."""
    perm = np.asarray(perm)
    return replace(c, offsets=c.offsets[perm], caplens=c.caplens[perm], summary=c.summary[perm], layers=c.layers[perm],
                   keep=None if c.keep is None else c.keep[perm])


def mixed(rng, n: int, big_every: int = 3) -> list[bytes]:
    """n Ethernet packets: small and large UDP / TCP over IPv4 (plain, VLAN, options), now and then an ARP packet, an
    IPv6 fragment, a fragment, a DF packet."""
    out = []
    for k in range(n):
        kind = k % 41
        if kind == 13:
            out.append(dc.eth(ethertype=0x0806) + bytes(28))
        elif kind == 29:
            out.append(dc.ipv6_fragment(rng, k))
        elif kind == 37:
            out.append(v4(rng, k, 64, foff=128, mf=k % 2 == 0))
        else:
            pay = int(rng.choice([8, 28, 120, 128, 136, 600, 1480])) if k % big_every == 0 else int(rng.integers(8, 120))
            out.append(v4(rng, k, pay, ip_off=(14, 18, 22)[k % 3], hdr=(20, 24, 20, 60)[k % 4], df=kind == 5,
                          tcp=k % 5 == 0))
    return out


def clean_udp(rng, n: int, max_pay: int = 1472) -> list[bytes]:
    """The round trip's input: no DF bits, no trailers, correct IPv4 checksums, one (source, destination, id) each."""
    out = []
    for k in range(n):
        pay = int(rng.choice([8, 30, 64, 65, 200, 1000, max_pay]))
        out.append(v4(rng, k, pay, ip_off=18 if k % 4 == 0 else 14, hdr=24 if k % 7 == 0 else 20, tcp=k % 3 == 0))
    out[3 % n] = dc.eth(ethertype=0x0806) + bytes(28)
    return out


# ------------------------------------------------------------------ the families
OVERFLOWING: list[str] = []
JUMBO_AT = 40  # the jumbo datagram's place among the 63 minimum-size packets


def _over(c: Case) -> Case:
    OVERFLOWING.append(c.name)
    return c


def cases() -> list[Case]:
    OVERFLOWING.clear()
    out: list[Case] = []
    rng = np.random.default_rng(4242)
    # the IP payload around one and two fragment sizes, per fragment size, header length and encapsulation
    for fs in (8, 16, 128, 1480):
        pays = [fs - 1, fs, fs + 1, 2 * fs - 1, 2 * fs, 2 * fs + 1]
        for ip_off in (0, 14, 16, 18, 22):
            pk = [v4(rng, 7 * k + h, p, ip_off=ip_off, hdr=h) for k, p in enumerate(pays) for h in (20, 24, 60)]
            out.append(make(f"size{fs}_ipoff{ip_off}", pk, l2(ip_off)[1], frag_size=fs, out_misalign=(fs + ip_off) % 16))
    # the largest fragment size: every payload a header leaves room for fits (hdr + pay <= 65535), raw IP
    out.append(make("size65528", [v4(rng, 1, 65515, ip_off=0), v4(rng, 2, 65475, ip_off=0, hdr=60), v4(rng, 3, 9, ip_off=0)],
                    RAW, frag_size=65528))
    for mtu in (68, 576, 1500):
        pk = []
        for h in (20, 24, 60):
            f = (mtu - h) & ~7
            pk += [v4(rng, len(pk) + j, p, hdr=h, ip_off=(14, 18)[j % 2])
                   for j, p in enumerate(sorted({mtu - h - 1, mtu - h, mtu - h + 1, f - 1, f, f + 1, 2 * f - 1, 2 * f,
                                                  2 * f + 1, 5 * f + 3}))]
        out.append(make(f"mtu{mtu}", pk, mtu=mtu, src_misalign=mtu % 16))
    # every source alignment: 16 packets, packet k behind k unused bytes more
    pk = [v4(rng, k, 300 + k, hdr=(20, 24)[k % 2]) for k in range(16)]
    lens = np.array([len(p) for p in pk], np.uint32)
    offs, pos = np.zeros(16, np.uint64), 1
    for k in range(16):
        pos += (k - pos) % 16 + 16 * (k % 2)  # packet k starts k bytes past a 16-B boundary
        offs[k] = pos
        pos += int(lens[k])
    data = np.full(pos + 5, 0xEE, np.uint8)
    for o, p in zip(offs, pk):
        data[int(o):int(o) + len(p)] = np.frombuffer(p, np.uint8)
    assert [int(o) % 16 for o in offs] == list(range(16))
    gapped = over("gapped_alignments", data, offs, lens, frag_size=16)
    out.append(gapped)
    out.append(replace(permuted(gapped, np.arange(16)[::-1]), name="reversed", frag_size=64, out_misalign=7))
    # overlapping sources: every packet twice, and the IP packet inside it as a packet of its own would not parse as
    # Ethernet: a second descriptor that starts inside the first (its records are the oracle's, whatever they say)
    twice = np.repeat(np.arange(16), 2)
    o2, l2_ = offs[twice].copy(), lens[twice].copy()
    o2[1::4] += 3
    l2_[1::4] -= 3
    out.append(over("overlapping", data, o2, l2_, frag_size=128))
    # a trailer behind the IP payload (dropped from every fragment), a capture cut inside the IP payload
    out.append(make("trailer", [v4(rng, 1, 300, trailer=bytes(range(1, 9))), v4(rng, 2, 40, trailer=b"\0" * 6),
                                v4(rng, 3, 128, trailer=b"\1\2"), v4(rng, 4, 129, trailer=b"\1\2\3")], frag_size=128))
    out.append(make("cut_capture", [v4(rng, 1, 1000, cut=300), v4(rng, 2, 1000, cut=999), v4(rng, 3, 300, cut=1),
                                    v4(rng, 4, 137, cut=9), v4(rng, 5, 200, cut=190)], frag_size=128))
    # expansion: 185 fragments (more than a wave) of one packet; 8,190 (more output packets than a block has sources) of
    # one jumbo datagram among 63 minimum-size packets
    out.append(make("expand_185", [v4(rng, 1, 8), v4(rng, 2, 1480), v4(rng, 3, 8)], frag_size=8))
    pk = [v4(rng, k, 8, ip_off=0) for k in range(64)]
    pk[JUMBO_AT] = v4(rng, 999, 65515, ip_off=0)
    jumbo = make("jumbo_8190", pk, RAW, frag_size=8, out_misalign=11)
    out.append(jumbo)
    out.append(replace(jumbo, name="jumbo_only_fragments", copy_rest=False, mtu=68, frag_size=0))
    # batch sizes around the tile and the block
    for n in (1, 63, 64, 65, 1023, 1024, 1025, 2049):
        out.append(make(f"n{n}", mixed(rng, n), frag_size=128, src_misalign=n % 16, out_misalign=(3 * n) % 16))
    # a block that puts out nothing between blocks that do
    pk = mixed(rng, BLOCK) + [v4(rng, k, 8 + k % 90) for k in range(BLOCK)] + mixed(rng, 200)
    out.append(make("empty_block", pk, frag_size=128, copy_rest=False))
    # keep masks; the dispositions
    base = make("keep_all", mixed(rng, 300), frag_size=64)
    out.append(base)
    out.append(replace(base, name="keep_none", keep=np.zeros(300, np.uint8)))
    out.append(replace(base, name="keep_alternating", keep=(np.arange(300) % 2 * 0x80).astype(np.uint8)))
    out.append(replace(base, name="keep_alternating_only", keep=(np.arange(300) % 2 == 0).astype(np.uint8),
                       copy_rest=False, use_brief=True))
    pk = [v4(rng, 1, 400, df=True), v4(rng, 2, 400), v4(rng, 3, 40, df=True), v4(rng, 4, 128, mf=True),
          v4(rng, 5, 128, foff=128, mf=True), v4(rng, 6, 77, foff=256), v4(rng, 7, 400, foff=8, df=True),
          dc.ipv6_fragment(rng, 8), dc.eth(ethertype=0x0806) + bytes(28),
          dc.eth(ethertype=0x86DD) + struct.pack(">IHBB", 0x60000000, 300, 17, 64) + bytes(32) + dc.udp_datagram(rng, 300)]
    out.append(make("dispositions_df0", pk, frag_size=64))
    out.append(make("dispositions_df1", pk, frag_size=64, honor_df=True))
    out.append(make("dispositions_mtu_df1", pk, mtu=100, honor_df=True, copy_rest=False))
    # records that point outside the packet or at no header: never followed
    c = make("bad_records", [v4(rng, k, 300, hdr=(20, 24)[k % 2]) for k in range(12)], frag_size=64)
    ip = [int(np.nonzero(c.layers[i]["proto"] == P_IPV4)[0][0]) for i in range(c.n)]
    c.layers["data_len"][0, ip[0]] += 1          # one byte past the capture
    c.layers["offset"][1, ip[1]] = 60000
    c.layers["hdr_len"][2, ip[2]] = 19
    c.layers["hdr_len"][3, ip[3]] = 61
    c.layers["hdr_len"][4, ip[4]] = c.layers["data_len"][4, ip[4]] + 1
    c.layers["data_len"][5, ip[5]] = 0xFFFF
    c.summary["n_layers"][6] = ip[6]             # the chain stops in front of the IPv4 layer
    c.layers["data_len"][7, ip[7]] -= 100        # shorter: followed, inside the packet
    c.layers["offset"][8, ip[8]] += 4            # elsewhere inside the packet: followed (whatever bytes lie there)
    c.layers["data_len"][8, ip[8]] -= 4
    c.summary["n_layers"][9] = 200               # more layers than the row holds: the first max_layers count
    out.append(c)
    # bad descriptors, the 64-bit wrap among them
    for rest in (True, False):
        out.append(mc.with_bad_descriptors(make(f"bad_desc_rest{int(rest)}", mixed(rng, 700), frag_size=128,
                                                copy_rest=rest)))
    # capacities: exact and one short; index-only; no optional columns; nothing to do
    base = make("cap", mixed(rng, 500), frag_size=64)
    op, ob = needs(base)
    assert op > base.n + 200
    for nm, kw, over_ in (("cap_exact", dict(data_cap=ob, max_packets=op), False),
                          ("cap_short1", dict(data_cap=ob - 1), True), ("maxp_short1", dict(max_packets=op - 1), True),
                          ("cap_zero", dict(data_cap=0), True), ("maxp_zero_sizing", dict(max_packets=0, index_only=True), True),
                          ("index_only", dict(index_only=True), False),
                          ("index_only_cap_ignored", dict(index_only=True, data_cap=3), False),
                          ("index_only_maxp_short1", dict(index_only=True, max_packets=op - 1), True),
                          ("no_columns", dict(want_index=False, want_columns=False), False)):
        c = replace(base, name=nm, **kw)
        out.append(_over(c) if over_ else c)
    out.append(make("n0", [], frag_size=8))
    out.append(make("nothing_split", [v4(rng, k, 8 + k % 50) for k in range(130)], frag_size=1480))
    out.append(make("nothing_out", [v4(rng, k, 8 + k % 50) for k in range(130)], mtu=1500, copy_rest=False))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
