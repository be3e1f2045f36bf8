"""Case generators, the model and runners for pcppx_frag6_device / pcppx_frag6_reference (tests/test_frag6.py).

The cases, buffers and IPv4 packet builders are those of tests/frag_cases.py with three more fields: the spec's
families, ids and id_base. brute() restates include/pcppx.h's frag6 contract as a per-packet Python loop; run_reference() and
run_device() give the same Buffers from pcppx_frag6_reference and pcppx_frag6_device, every buffer pre-filled with 0xA5
and over-allocated.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, fields, replace

import numpy as np

import defrag6_cases as d6
import defrag_cases as dc
import frag_cases as fc
import mover_cases as mc
from frag_cases import BLOCK, ETH, FIELDS, ML, Buffers, alloc, assert_same, assert_untouched, output_batch  # noqa: F401
from pcapplusplus_amd import abi

P_IPV4, P_IPV6 = 2, 3
V4, V6 = abi.FRAG_FAM_V4, abi.FRAG_FAM_V6
EXT_TYPES = (0, 43, 44, 51, 60)
MAX_EXT = abi.FRAG6_MAX_EXT


@dataclass
class Case(fc.Case):
    families: int = V4 | V6
    ids: np.ndarray | None = None  # u32[n]; None: id_base + i
    id_base: int = 0

    def cap(self) -> int:
        return needs(self)[1] if self.data_cap is None else self.data_cap

    def maxp(self) -> int:
        return needs(self)[0] if self.max_packets is None else self.max_packets

    def ident(self, i: int) -> int:
        return int(self.ids[i]) if self.ids is not None else (self.id_base + i) & 0xFFFFFFFF


def widen(c: fc.Case, families: int, **kw) -> Case:
    """A frag case as a frag6 one."""
    return Case(**{f.name: getattr(c, f.name) for f in fields(c)}, families=families, **kw)


def make(name: str, packets: list[bytes], families: int = V4 | V6, ids=None, id_base: int = 0, linktype: int = ETH,
         **kw) -> Case:
    return widen(fc.make(name, packets, linktype, **kw), families, ids=ids, id_base=id_base)


# ------------------------------------------------------------------ the contract, one packet at a time
def walk(ip: bytes, hdr: int):
    """The extension walk over ip[40:hdr]: ("not_ip" | "left" | "ok", nh_at relative to the header, fragmented)."""
    nh, at, rel, frag, steps = ip[6], 40, 6, False, 0
    while at < hdr:
        if nh not in EXT_TYPES or at + 2 > hdr:
            return "not_ip", rel, frag
        if steps == MAX_EXT:
            return "left", rel, frag
        steps += 1
        frag = frag or nh == 44
        ext = 8 if nh == 44 else (ip[at + 1] + 2) * 4 if nh == 51 else (ip[at + 1] + 1) * 8
        rel, nh, at = at, ip[at], at + ext
    return ("ok" if at == hdr else "not_ip"), rel, frag


PLAIN = (1, 9, 19)  # pcpp::Ethernet, VLAN, SLL: the layers an IPv6 candidate may have ahead of it


def ahead(c: Case, i: int):
    """The layers recorded ahead of packet i's first IPv6 layer."""
    rows = [c.layers[i, k] for k in range(min(int(c.summary["n_layers"][i]), ML))]
    k6 = next((k for k, L in enumerate(rows) if int(L["proto"]) == P_IPV6), len(rows))
    return rows[:k6], rows


def type_fields(c: Case, i: int, ip_off: int) -> list[int]:
    """The packet offsets of the type fields the reference sets to 0x8100: the two bytes ahead of every VLAN layer that
    follows a layer ahead of the IPv6 one."""
    front, rows = ahead(c, i)
    out = []
    for k in range(len(front)):
        if k + 1 < len(rows) and int(rows[k + 1]["proto"]) == 9 and 2 <= int(rows[k + 1]["offset"]) <= ip_off:
            out.append(int(rows[k + 1]["offset"]) - 2)
    return out


def plan(c: Case):
    """Per source packet: (disposition, (ip_off, hdr, pay, fs, v6, nh_at) for a SPLIT packet)."""
    out = []
    data_len = c.dlen()
    for i in range(c.n):
        off, cap = int(c.offsets[i]), int(c.caplens[i])
        if off + cap > data_len:
            out.append((abi.FRAG_BAD_DESC, None))
            continue
        if c.keep is not None and int(c.keep[i]) == 0:
            out.append((abi.FRAG_UNSELECTED, None))
            continue
        rows = [c.layers[i, k] for k in range(min(int(c.summary["n_layers"][i]), ML))]
        l4 = next((L for L in rows if int(L["proto"]) == P_IPV4), None)
        l6 = next((L for L in rows if int(L["proto"]) == P_IPV6), None)
        if l4 is not None or not c.families & V6:
            geo = fc.ipv4_layer(c, i, cap) if c.families & V4 else None
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
            out.append((d, (o, h, pay, fs, False, 0)))
            continue
        if l6 is None:
            out.append((abi.FRAG_NOT_IP, None))
            continue
        o, h, dl = int(l6["offset"]), int(l6["hdr_len"]), int(l6["data_len"])
        if not (40 <= h <= dl and o + dl <= cap):
            out.append((abi.FRAG_NOT_IP, None))
            continue
        pay = dl - h
        verdict, rel, fragmented = walk(c.data[off + o:off + o + h].tobytes(), h)
        fs = c.frag_size if c.frag_size else (c.mtu - h - 8) & ~7
        if verdict == "not_ip":
            d = abi.FRAG_NOT_IP
        elif verdict == "left" or any(int(L["proto"]) not in PLAIN for L in ahead(c, i)[0]):
            d = abi.FRAG_LEFT
        elif fragmented:
            d = abi.FRAG_ALREADY
        elif (pay <= fs) if c.frag_size else (h + pay <= c.mtu):
            d = abi.FRAG_FITS
        elif not c.frag_size and c.mtu < h + 16:
            d = abi.FRAG_LEFT
        else:
            d = abi.FRAG_SPLIT
        out.append((d, (o, h, pay, fs, True, o + rel)))
    return out


def fragment6_bytes(src: bytes, o: int, h: int, pay: int, fs: int, nh_at: int, j: int, count: int, ident: int,
                    types=()) -> bytes:
    piece = src[o + h + j * fs:o + h + min((j + 1) * fs, pay)]
    head = bytearray(src[:o + h])
    for at in types:
        head[at:at + 2] = b"\x81\x00"
    fh = struct.pack(">BBHI", head[nh_at], 0, (j * fs) | (1 if j < count - 1 else 0), ident)
    head[nh_at] = 44
    head[o + 4:o + 6] = struct.pack(">H", h - 40 + 8 + len(piece))
    return bytes(head) + fh + piece


def rows_of(c: Case, plans=None):
    """The output packets in order: (source, fragment number, bytes); and the per-source counts."""
    plans = plan(c) if plans is None else plans
    rows, counts = [], []
    for i, (d, geo) in enumerate(plans):
        before = len(rows)
        off = int(c.offsets[i])
        if d == abi.FRAG_SPLIT:
            o, h, pay, fs, v6, nh_at = geo
            src = c.data[off:off + int(c.caplens[i])].tobytes()
            count = -(-pay // fs)
            if v6:
                types = type_fields(c, i, o)
                rows += [(i, j, fragment6_bytes(src, o, h, pay, fs, nh_at, j, count, c.ident(i), types))
                         for j in range(count)]
            else:
                rows += [(i, j, fc.fragment_bytes(src, o, h, pay, fs, j, count)) for j in range(count)]
        elif d != abi.FRAG_BAD_DESC and c.copy_rest:
            rows.append((i, 0, c.data[off:off + int(c.caplens[i])].tobytes()))
        counts.append(len(rows) - before)
    return rows, counts


_NEEDS: dict[tuple, tuple] = {}


def needs(c: Case) -> tuple[int, int]:
    """(output packets, output bytes) of the case's rule over its batch, whatever its capacities."""
    key = (id(c.data), id(c.offsets), id(c.caplens), id(c.layers), id(c.summary), id(c.keep), c.frag_size, c.mtu,
           c.copy_rest, c.honor_df, c.data_len, c.families)
    if key not in _NEEDS:
        rows, _ = rows_of(c)
        _NEEDS[key] = (len(rows), sum(len(r[2]) for r in rows), c)  # c kept alive: the ids stay its own
    return _NEEDS[key][:2]


def brute(c: Case) -> Buffers:
    """include/pcppx.h's frag6 contract restated."""
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
def spec_of(c: Case, keep_addr, ids_addr) -> abi.Frag6Spec:
    return abi.make_frag6_spec(c.frag_size, c.mtu, c.families, ids_addr, c.id_base, keep_addr, c.copy_rest, c.honor_df)


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, c.linktype, 0)
    rec, alive = fc.host_records(c)
    keep = None if c.keep is None else np.ascontiguousarray(c.keep if c.n else np.zeros(1, np.uint8))
    ids = None if c.ids is None else np.ascontiguousarray(c.ids if c.n else np.zeros(1, np.uint32)).astype(np.uint32)
    opt = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = abi.Fragmented(opt(out.data), c.cap(), out.offsets.ctypes.data, out.caplens.ctypes.data, opt(out.index),
                       opt(out.frag_no), opt(out.counts), opt(out.disposition), c.maxp(), 0, out.totals.ctypes.data)
    abi.frag6_reference(b, rec, ML, spec_of(c, opt(keep), opt(ids)), o)
    del alive
    return out


class DeviceRun(fc.DeviceRun):
    """frag_cases.DeviceRun through pcppx_frag6_device."""

    def __init__(self, c: Case, device: str = "cuda:0", source=None):
        super().__init__(c, device, source)
        ids = None if c.ids is None else np.ascontiguousarray(c.ids if c.n else np.zeros(1, np.uint32))
        self.ids = None if ids is None else self.up(ids.astype(np.uint32).view(np.int32))

    def launch(self, engine, stream: int) -> None:
        c = self.c
        spec = spec_of(c, None if self.keep is None else abi.ptr(self.keep),
                       None if self.ids is None else abi.ptr(self.ids))
        engine.frag6_device(self.data, self.offsets, self.caplens, c.n, c.linktype, self.layers, ML, spec, self.d_off,
                            self.d_cap, self.d_tot, c.maxp(), self.d_data, c.cap(), self.d_idx, self.d_no, self.d_cnt,
                            self.d_disp, stream, data_len=self.data_len, summary=self.summary, brief=self.brief)


def run_device(engine, c: Case, device: str = "cuda:0", source=None) -> Buffers:
    import torch

    run = DeviceRun(c, device, source)
    run.launch(engine, torch.cuda.current_stream(device).cuda_stream)
    return run.result()


# ------------------------------------------------------------------ packets
def l2_6(ip_off: int, outer: int = 0x8100, inner: int = 0x8100) -> bytes:
    """Ethernet and (ip_off - 14) / 4 VLAN tags in front of an IPv6 header; outer / inner: the type fields ahead of the
    first and the second tag."""
    mac = bytes.fromhex("020000000001") + bytes.fromhex("020000000002")
    tags = {14: b"", 18: struct.pack(">HH", outer, 5), 22: struct.pack(">HHHH", outer, 7, inner, 5)}[ip_off]
    return mac + tags + struct.pack(">H", 0x86DD)


def sll_6(tags: int, first: int = 0x8100, second: int = 0x8100) -> bytes:
    """A Linux cooked header and `tags` VLAN tags in front of an IPv6 header."""
    types = [first, second][:tags] + [0x86DD]
    out = struct.pack(">HHH8sH", 0, 1, 6, bytes.fromhex("0200000000010000"), types[0])
    for t in range(tags):
        out += struct.pack(">HH", 5 + t, types[t + 1])
    return out


def ext(kind: int, nh: int, units: int = 1) -> bytes:
    """One extension header naming nh as the next one. Hop-by-Hop (0), Routing (43) and Destination (60): units * 8
    bytes; AH (51): (units + 2) * 4 bytes (its length byte counts 4-byte words less two); Fragment (44): 8 bytes."""
    if kind == 44:
        return d6.frag_hdr(nh, 0, False, 0xABCD0123)
    if kind == 51:
        return bytes([nh, units, 0, 0]) + struct.pack(">II", 0x1001, 7) + bytes(range(0x40, 0x40 + (units - 1) * 4))
    if kind == 43:
        return bytes([nh, units - 1, 0, 0]) + bytes(units * 8 - 4)
    return d6.opts_hdr(nh, units)


def chain(kinds, proto: int) -> tuple[int, bytes]:
    """(the fixed header's next-header value, the extension bytes) of extensions (kind, units) ahead of `proto`."""
    kinds = [(k, 1) if isinstance(k, int) else k for k in kinds]
    body = b""
    for n, (k, u) in enumerate(kinds):
        body += ext(k, kinds[n + 1][0] if n + 1 < len(kinds) else proto, u)
    return (kinds[0][0] if kinds else proto), body


def v6(rng, k: int, pay: int, ip_off: int = 14, exts=(), tcp: bool = False, trailer: bytes = b"", cut: int = 0,
       plen: int | None = None, outer: int = 0x8100, inner: int = 0x8100, l2: bytes | None = None) -> bytes:
    """An IPv6 packet with `pay` bytes behind its extensions (UDP, or TCP, where the header fits)."""
    if tcp and pay >= 20:
        l4 = struct.pack(">HHIIBBHHH", 1024 + k % 999, 80, k, 0, 0x50, 0x10, 512, 0, 0) + \
            rng.integers(0, 256, pay - 20, dtype=np.uint8).tobytes()
    elif pay >= 8:
        l4 = dc.udp_datagram(rng, pay, 1024 + k % 50, 2000 + k % 7)
    else:
        l4 = rng.integers(0, 256, pay, dtype=np.uint8).tobytes()
    nh, body = chain(exts, 6 if tcp else 17)
    front = l2_6(ip_off, outer, inner) if l2 is None else l2
    p = front + d6.ipv6(0x100 + k % 251, 0x200 + k // 251, nh, body + l4, plen) + trailer
    return p[:len(p) - cut] if cut else p


def six_in_four(rng, k: int, pay: int) -> bytes:
    inner = v6(rng, k, pay)[14:]
    return dc.eth() + dc.ipv4(0x0A000001, 0x0B000001 + k, k, inner, proto=41)


def four_in_six(rng, k: int, pay: int, exts=()) -> bytes:
    inner = fc.v4(rng, k, pay, ip_off=0)
    nh, body = chain(exts, 4)
    return l2_6(14) + d6.ipv6(1, 2 + k, nh, body + inner)


def mixed(rng, n: int) -> list[bytes]:
    """fc.mixed()'s IPv4 / ARP / fragment traffic with every fourth packet an IPv6 one: small and large, plain, tagged
    (now and then with 802.1ad type fields), with a Hop-by-Hop header, with Hop-by-Hop / Routing / Destination, with an
    AH."""
    out = fc.mixed(rng, n)
    shapes = ((), (0,), (), (0, 43, 60), ((51, 1),), ((60, 2),))
    for k in range(1, n, 4):
        pay = int(rng.choice([8, 28, 120, 128, 136, 600, 1400])) if k % 3 else int(rng.integers(8, 120))
        out[k] = v6(rng, k, pay, ip_off=(14, 18, 22)[k % 3], exts=shapes[k % len(shapes)], tcp=k % 5 == 0,
                    outer=0x88A8 if k % 16 == 5 else 0x8100, inner=0x88A8 if k % 32 == 13 else 0x8100)
    return out


# ------------------------------------------------------------------ the recorded shapes
def quirk_cases(rng=None) -> list[Case]:
    """The crafted packets whose fragments tests/golden/frag6/expected.npz records from the reference's own routine
    (copy the RawPacket, removeAllLayersAfter, addLayer(PayloadLayer), addExtension(IPv6FragmentationHeader),
    computeCalculateFields). One packet per case; the ids are the case's id_base + 0."""
    rng = np.random.default_rng(606) if rng is None else rng
    q = lambda name, p, fs, ident: make(name, [p], frag_size=fs, id_base=ident)  # noqa: E731
    out = [
        q("plain", v6(rng, 1, 300), 128, 0x01020304),
        q("vlan1", v6(rng, 2, 200, ip_off=18), 64, 0xFFFFFFFF),
        q("vlan2", v6(rng, 3, 200, ip_off=22), 64, 0),
        q("hbh_tcp", v6(rng, 4, 260, exts=(0,), tcp=True), 128, 0x80000000),
        q("hbh_routing_dst", v6(rng, 5, 100, exts=(0, (43, 3), (60, 2))), 40, 7),
        q("ah_12", v6(rng, 6, 90, exts=((51, 1),)), 32, 0xDEADBEEF),
        q("ah_24_behind_hbh", v6(rng, 7, 90, ip_off=18, exts=(0, (51, 4))), 32, 0x11223344),
        q("trailer", v6(rng, 8, 150, trailer=bytes(range(0xE0, 0xEB))), 64, 9),
        # the payload-length field smaller than the capture: the layer is clamped to payloadLength + hdr, which counts
        # the 16 extension bytes twice, so 16 bytes more than the field says are payload
        q("plen_small", v6(rng, 9, 200, exts=(0, 60), plen=16 + 120), 48, 10),
        q("plen_small_no_ext", v6(rng, 10, 200, plen=120), 48, 11),
        q("plen_large", v6(rng, 11, 200, exts=(0,), plen=4000), 64, 12),
        q("pay_eq_fs", v6(rng, 12, 64), 64, 13),
        q("pay_fs_plus_1", v6(rng, 13, 65), 64, 14),
        q("pay_2fs", v6(rng, 14, 128, exts=(60,)), 64, 15),
        # the layers ahead: computeCalculateFields of Ethernet, VLAN and SLL sets the type field ahead of a VLAN layer
        # to 0x8100, so an 802.1ad tag (0x88A8) is renamed in every fragment
        q("qinq_88a8", v6(rng, 20, 200, ip_off=22, outer=0x88A8), 64, 21),
        q("inner_88a8", v6(rng, 21, 200, ip_off=22, inner=0x88A8, exts=(0,)), 64, 22),
        q("both_88a8", v6(rng, 22, 150, ip_off=22, outer=0x88A8, inner=0x88A8), 64, 23),
        q("one_tag_88a8", v6(rng, 23, 150, ip_off=18, outer=0x88A8), 64, 24),
    ]
    sll = lambda name, p, ident: make(name, [p], frag_size=64, id_base=ident, linktype=fc.SLL)  # noqa: E731
    out += [
        sll("sll_plain", v6(rng, 24, 150, l2=sll_6(0)), 25),
        sll("sll_88a8", v6(rng, 25, 150, l2=sll_6(1, 0x88A8)), 26),
        sll("sll_two_88a8", v6(rng, 26, 150, l2=sll_6(2, 0x88A8, 0x88A8), exts=(0,)), 27),
    ]
    return out


# ------------------------------------------------------------------ the families
OVERFLOWING: list[str] = []
JUMBO_AT = 40
GAP_HEADS = (54, 58, 62, 62 + 8, 54 + 24)  # ip_off + hdr of the gap-alignment cases


def _over(c: Case) -> Case:
    OVERFLOWING.append(c.name)
    return c


def gap_packets(rng, head: int, count: int) -> list[bytes]:
    """IPv6 packets with ip_off + hdr == head whose lengths step by one byte."""
    ip_off, exts = {54: (14, ()), 58: (18, ()), 62: (22, ()), 70: (22, (0,)), 78: (14, (0, (60, 2)))}[head]
    return [v6(rng, k, 40 + k, ip_off=ip_off, exts=exts) for k in range(count)]


def cases() -> list[Case]:
    OVERFLOWING.clear()
    out: list[Case] = []
    rng = np.random.default_rng(6006)
    for c in quirk_cases():
        out.append(c)
    # a layer ahead of the IPv6 header that is not Ethernet, VLAN or SLL: LEFT (an MPLS label; GRE behind IPv6 is the
    # outer IPv6 packet's payload and splits at the outer header)
    mpls = bytes.fromhex("020000000001") + bytes.fromhex("020000000002") + \
        struct.pack(">HI", 0x8847, (77 << 12) | 0x100 | 64)
    out.append(make("mpls_ahead", [v6(rng, 30, 300, l2=mpls), v6(rng, 31, 300)], frag_size=64))
    # the payload around one and two fragment sizes, per fragment size, extension chain and encapsulation
    for fs in (8, 16, 128, 1480):
        pays = [fs - 1, fs, fs + 1, 2 * fs - 1, 2 * fs, 2 * fs + 1]
        for ip_off in (14, 18, 22):
            pk = [v6(rng, 7 * k + u, p, ip_off=ip_off, exts=e)
                  for k, p in enumerate(pays) for u, e in enumerate(((), (0,), (0, 43, (51, 1))))]
            out.append(make(f"size{fs}_ipoff{ip_off}", pk, frag_size=fs, out_misalign=(fs + ip_off) % 16))
    # mtu mode: the packet around the mtu, the fragment size from mtu - hdr - 8; the LEFT rule where mtu < hdr + 16
    for mtu in (68, 576, 1500):
        pk = []
        for e in ((), (0,), ((60, 4),), ((51, 1),)):
            h = 40 + len(chain(e, 17)[1])
            f = max((mtu - h - 8) & ~7, 8)
            pk += [v6(rng, len(pk) + j, max(p, 1), exts=e, ip_off=(14, 18)[j % 2])
                   for j, p in enumerate(sorted({mtu - h - 1, mtu - h, mtu - h + 1, f - 1, f, f + 1, 2 * f, 2 * f + 1,
                                                  5 * f + 3}))]
        out.append(make(f"mtu{mtu}", pk, mtu=mtu, src_misalign=mtu % 16))
    # gap alignment: per head length, 24 packets whose lengths step by one, fragment sizes 8 and 24: the gap of the
    # fragments meets every destination residue mod 16 (test_gap_cases_cover_every_residue), straddling included
    for head in GAP_HEADS:
        for fs in (8, 24):
            out.append(make(f"gap_head{head}_fs{fs}", gap_packets(rng, head, 24), frag_size=fs, id_base=0xA0B0C0D0,
                            out_misalign=(head + fs) % 16, src_misalign=head % 16))
    # more than 64 and more than 1024 fragments of one packet: fs = 8 on the largest payload the capture allows
    pk = [v6(rng, k, 8) for k in range(64)]
    pk[JUMBO_AT] = v6(rng, 999, abi.MAX_CAPLEN - 14 - 40)
    out.append(make("jumbo", pk, frag_size=8, out_misalign=11))
    pk = [v6(rng, k, 8) for k in range(3)]
    pk[1] = v6(rng, 998, 8 * 150 + 3, exts=(0,))
    out.append(make("expand_151", pk, frag_size=8, copy_rest=False))
    # batch sizes around the tile and the block; both families, the three specs
    for n in (63, 1025, 2049):
        ids = (np.arange(n, dtype=np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
        out.append(make(f"n{n}", mixed(rng, n), frag_size=128, ids=ids, src_misalign=n % 16, out_misalign=(3 * n) % 16))
    base = make("mixed_v4v6", mixed(rng, 300), frag_size=64, id_base=0xFFFFFF00)  # the ids wrap at 2^32
    out.append(base)
    out.append(replace(base, name="mixed_v6", families=V6))
    out.append(replace(base, name="mixed_v4", families=V4))
    out.append(replace(base, name="mixed_mtu_brief", frag_size=0, mtu=200, use_brief=True, copy_rest=False))
    out.append(replace(base, name="keep_alternating", keep=(np.arange(300) % 2 * 0x80).astype(np.uint8)))
    # a block that puts out nothing between blocks that do
    pk = mixed(rng, BLOCK) + [v6(rng, k, 8 + k % 90) for k in range(BLOCK)] + mixed(rng, 200)
    out.append(make("empty_block", pk, frag_size=128, copy_rest=False))
    # family selection: one packet each
    for fam in (V4 | V6, V6, V4):
        out.append(make(f"six_in_four_f{fam}", [six_in_four(rng, 1, 300)], families=fam, frag_size=64))
        out.append(make(f"four_in_six_f{fam}", [four_in_six(rng, 2, 300, exts=(0,))], families=fam, frag_size=64))
    # the extension walk: 16 extensions are walked, 17 are LEFT; a fragment header anywhere in the chain: ALREADY
    out.append(make("ext16", [v6(rng, 1, 100, exts=(0,) + (60,) * 15)], frag_size=64))
    out.append(make("ext17", [v6(rng, 1, 100, exts=(0,) + (60,) * 16)], frag_size=64))
    pk = [v6(rng, 1, 100, exts=(44,)), v6(rng, 2, 100, exts=(0, 44, 60)), v6(rng, 3, 100, exts=(0,))]
    out.append(make("already", pk, frag_size=64))
    # mtu-mode LEFT: hdr = 40 + 8 * 6 = 88 > mtu - 16 = 84 (and a packet that fits is still FITS)
    pk = [v6(rng, 1, 100, exts=((60, 6),)), v6(rng, 2, 8, exts=((60, 2),)), v6(rng, 3, 100)]
    out.append(make("mtu_left", pk, mtu=100))
    # records that point outside the packet or at a chain the bytes do not hold: NOT_IP, never followed
    c = make("bad_records", [v6(rng, k, 300, exts=((0,) if k % 2 else ())) for k in range(10)], frag_size=64)
    ip = [int(np.nonzero(c.layers[i]["proto"] == P_IPV6)[0][0]) for i in range(c.n)]
    c.layers["data_len"][0, ip[0]] += 1          # one byte past the capture
    c.layers["offset"][1, ip[1]] = 60000
    c.layers["hdr_len"][2, ip[2]] = 39
    c.layers["hdr_len"][3, ip[3]] += 8           # the chain ends short of hdr (UDP is no extension)
    c.layers["hdr_len"][4, ip[4]] = c.layers["data_len"][4, ip[4]] + 1
    c.layers["hdr_len"][5, ip[5]] -= 4           # an extension that crosses hdr
    c.summary["n_layers"][6] = ip[6]             # the chain stops in front of the IPv6 layer
    c.layers["data_len"][7, ip[7]] -= 100        # shorter: followed, inside the packet
    c.layers["hdr_len"][9, ip[9]] = 41           # no room for an extension's two bytes
    out.append(c)
    out.append(mc.with_bad_descriptors(make("bad_desc", mixed(rng, 400), frag_size=128)))
    # capacities: exact and one short; index-only; the sizing call; no optional columns; nothing to do
    base = make("cap", mixed(rng, 300), frag_size=64)
    op, ob = needs(base)
    for nm, kw, over_ in (("cap_exact", dict(data_cap=ob, max_packets=op), False),
                          ("cap_short1", dict(data_cap=ob - 1), True), ("maxp_short1", dict(max_packets=op - 1), True),
                          ("maxp_zero_sizing", dict(max_packets=0, index_only=True), True),
                          ("index_only", dict(index_only=True), False),
                          ("no_columns", dict(want_index=False, want_columns=False), False),
                          ("copy_rest0", dict(copy_rest=False), False)):
        c = replace(base, name=nm, **kw)
        out.append(_over(c) if over_ else c)
    out.append(make("n0", [], frag_size=8))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
