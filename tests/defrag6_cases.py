"""Case generators, models and runners for pcppx_defrag6_device / pcppx_defrag6_reference (tests/test_defrag6.py).

The cases, buffers and packet builders are those of tests/defrag_cases.py with one more field, the spec's families.
brute() restates include/pcppx.h's defrag6 contract as a per-packet Python loop; run_reference() and run_device() give
the same Buffers from pcppx_defrag6_reference and pcppx_defrag6_device, every buffer pre-filled and over-allocated.

stream() is the second, independent model: defrag_cases.stream()'s processPacket machine for both families, its IPv6
finish written as the reference's own steps (the native 16-bit store of IPReassembly.cpp:476, the parse that clamps
the layer, removeAllExtensions, computeCalculateFields) rather than as the contract's closed formula.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, fields, replace

import numpy as np

import defrag_cases as dc
import mover_cases as mc
from defrag_cases import BLOCK, FIELDS, ML, Buffers, alloc, assert_same, assert_untouched, reassembled  # noqa: F401
from pcapplusplus_amd import abi

P_IPV4, P_IPV6 = 2, 3
V4, V6 = abi.DEFRAG_FAM_V4, abi.DEFRAG_FAM_V6
EXT_TYPES = (0, 43, 44, 51, 60)


@dataclass
class Case(dc.Case):
    families: int = V4 | V6


def make(name: str, packets: list[bytes], families: int = V4 | V6, **kw) -> Case:
    c = dc.make(name, packets, **kw)
    return Case(**{f.name: getattr(c, f.name) for f in fields(c)}, families=families)


def widen(c: dc.Case, families: int) -> Case:
    """A defrag case as a defrag6 one."""
    return Case(**{f.name: getattr(c, f.name) for f in fields(c)}, families=families)


# ------------------------------------------------------------------ the contract, one packet at a time
def candidates(c: Case, families: int | None = None):
    """Per packet: ("bad" | "pass" | "left" | "cand", (ip_off, hdr, len, v6) for a candidate). With families = V4 an
    IPv6 fragment is no candidate; else the fragments of both families are."""
    fam = c.families if families is None else families
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
        v6 = bool(st & abi.IPR_F_IPV6)
        if not (v6 and fam == V4):
            for k in range(min(int(c.summary["n_layers"][i]), ML)):
                L = c.layers[i, k]
                if int(L["proto"]) != (P_IPV6 if v6 else P_IPV4):
                    continue
                o, h, d = int(L["offset"]), int(L["hdr_len"]), int(L["data_len"])
                if h >= (48 if v6 else 20) and h <= d and o + d <= cap:
                    kind, geo = "cand", (o, h, d - h, v6)
                break
        out.append((kind, geo))
    return out


def walk_chain(ip: bytes, hdr: int):
    """(ok, nh): the extensions ip[40:hdr] walked from the fixed header's next-header byte."""
    nh, at, frag = ip[6], 40, False
    while at + 2 <= hdr and nh in EXT_TYPES:
        frag = frag or nh == 44
        ext = 8 if nh == 44 else (ip[at + 1] + 2) * 4 if nh == 51 else (ip[at + 1] + 1) * 8
        nh, at = ip[at], at + ext
    return at == hdr and frag and nh not in EXT_TYPES, nh


def patched6(pkt: bytearray, ip_off: int, hdr: int, total: int, nh: int) -> bytes:
    """The reassembled IPv6 packet's fields: the clamped payload length and the next header."""
    swapped = struct.unpack("<H", struct.pack(">H", (total + hdr) & 0xFFFF))[0]
    pkt[ip_off + 4:ip_off + 6] = struct.pack(">H", min(total, swapped))
    pkt[ip_off + 6] = nh
    return bytes(pkt)


def brute(c: Case) -> Buffers:
    """include/pcppx.h's defrag6 contract restated."""
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
    packets = {}  # completing member -> (sorted members, total, nh)
    for g in groups.values():
        g = sorted(g, key=lambda i: (int(c.info["frag_offset"][i]), i))
        if not 2 <= len(g) <= dc.MAX_FRAGS:
            continue
        o0, h0, _, v6 = kinds[g[0]][1]
        total, clean = 0, True
        for k, i in enumerate(g):
            ln = kinds[i][1][2]
            last = bool(int(c.info["ip_status"][i]) & abi.IPR_F_LAST)
            clean = clean and ln > 0 and int(c.info["frag_offset"][i]) == total and last == (k == len(g) - 1)
            clean = clean and kinds[i][1][3] == v6  # one family
            total += ln
        if not clean or o0 + h0 + total > abi.MAX_CAPLEN or h0 + total > 65535 or not c.families & (V6 if v6 else V4):
            continue
        nh = 0
        if v6:
            s = int(c.offsets[g[0]]) + o0
            ok, nh = walk_chain(c.data[s:s + h0].tobytes(), h0)
            if not ok:
                continue
        for i in g:
            d[i] = abi.DEFRAG_MERGED
        d[max(g)] = abi.DEFRAG_MERGED_LAST
        packets[max(g)] = (g, total, nh)
    rows = []  # (source, first, frags, bytes)
    for i in range(c.n):
        if d[i] == abi.DEFRAG_MERGED_LAST:
            g, total, nh = packets[i]
            o0, h0, l0, v6 = kinds[g[0]][1]
            src = int(c.offsets[g[0]])
            pkt = bytearray(c.data[src:src + o0 + (40 if v6 else h0)].tobytes())
            for m in g:
                o, h, ln, _ = kinds[m][1]
                s = int(c.offsets[m]) + o + h
                pkt += c.data[s:s + ln].tobytes()
            assert len(pkt) == o0 + (40 if v6 else h0) + total
            rows.append((i, g[0], len(g), patched6(pkt, o0, h0, total, nh) if v6 else dc.patched(pkt, o0, h0, total)))
        elif c.passthrough and d[i] in (abi.DEFRAG_PASS, abi.DEFRAG_LEFT):
            s = int(c.offsets[i])
            rows.append((i, i, 0, c.data[s:s + int(c.caplens[i])].tobytes()))
    nbytes = sum(len(r[3]) for r in rows)
    out.totals[:5] = (len(rows), nbytes, len(packets), sum(len(p[0]) for p in packets.values()),
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
def _parse_extensions(ip: bytes, data_len: int):
    """parseExtensions (IPv6Layer.cpp:79-147) over a layer of data_len bytes: (the extensions' length, the last one's
    next-header byte or None)."""
    nh, at, last = ip[6], 40, None
    while at <= data_len - 2 and nh in EXT_TYPES:
        ext = 8 if nh == 44 else (ip[at + 1] + 2) * 4 if nh == 51 else (ip[at + 1] + 1) * 8
        last = nh = ip[at]
        at += ext
    return at - 40, last


def finish6(data: bytearray, ip_off: int, cur: int) -> bytes:
    """IPReassembly.cpp:472-496 for an IPv6 packet of cur payload bytes, step by step."""
    ext, _ = _parse_extensions(bytes(data[ip_off:]), len(data) - ip_off)  # the temporary packet of :474
    data[ip_off + 4:ip_off + 6] = struct.pack("<H", (cur + 40 + ext) & 0xFFFF)  # :476, no htobe16
    ip = bytes(data[ip_off:])
    data_len = len(ip)
    ext, last = _parse_extensions(ip, data_len)  # the parse of :481 ...
    data_len = min(data_len, struct.unpack(">H", ip[4:6])[0] + 40 + ext)  # ... and its clamp (IPv6Layer.cpp:37-39)
    if last is not None:  # removeAllExtensions
        data[ip_off + 6] = last
    del data[ip_off + 40:ip_off + 40 + ext]
    data_len -= ext
    data[ip_off + 4:ip_off + 6] = struct.pack(">H", (data_len - 40) & 0xFFFF)  # computeCalculateFields
    return bytes(data)


def stream(c: Case, order=None) -> dict[int, tuple[bytes, int]]:
    """defrag_cases.stream() over the fragments of both families (the reference's table holds both, whatever the spec
    asks for): {position in order: (the packet returned there with REASSEMBLED, its first fragment's source number)}.
    An entry is of the family of the fragment that created it (IPFragmentData's packetKey)."""
    kinds = candidates(c, V4 | V6)
    table: dict[int, dc._Entry] = {}
    out = {}
    for at, i in enumerate(range(c.n) if order is None else order):
        kind, geo = kinds[i]
        if kind != "cand":
            continue
        ip_off, hdr, ln, v6 = geo
        key = int(c.info["ip_key"][i])
        st = int(c.info["ip_status"][i])
        foff = int(c.info["frag_offset"][i])
        src = int(c.offsets[i])
        payload = c.data[src + ip_off + hdr:src + ip_off + hdr + ln].tobytes()
        if key not in table:
            table[key] = dc._Entry()
            table[key].v6 = v6
        e = table[key]
        got_last = False
        if st & abi.IPR_F_FIRST:
            if e.data is not None:  # duplicated first fragment
                continue
            e.data = bytearray(c.data[src:src + ip_off + hdr + ln].tobytes())
            e.cur, e.geo, e.first = ln, (ip_off, hdr), i
            got_last = dc._match_out_of_order(e)
        elif e.cur == foff:
            if e.data is None:  # malformed: not the first fragment, but offset 0
                continue
            e.data += payload
            e.cur += ln
            got_last = True if st & abi.IPR_F_LAST else dc._match_out_of_order(e)
        elif foff > e.cur:
            e.ooo.append([foff, payload, bool(st & abi.IPR_F_LAST)])
            continue
        if got_last:
            pkt = finish6(e.data, e.geo[0], e.cur) if e.v6 else dc.patched(e.data, e.geo[0], e.geo[1], e.cur)
            out[at] = (pkt, e.first)
            del table[key]
    return out


# ------------------------------------------------------------------ runners
def _spec(c: Case) -> abi.Defrag6Spec:
    return abi.make_defrag6_spec(c.passthrough, c.max_fragments, c.families)


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, 1, 0)
    rec, keep = dc._records(c)
    info = np.ascontiguousarray(c.info) if c.n else np.zeros(1, abi.REASM_DTYPE)
    opt = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = abi.Defragged(opt(out.data), c.cap(), out.offsets.ctypes.data, out.caplens.ctypes.data, opt(out.index),
                      opt(out.first), opt(out.frags), opt(out.disposition), c.maxp(), 0, out.totals.ctypes.data)
    abi.defrag6_reference(b, rec, ML, info.ctypes.data, _spec(c), o)
    del keep
    return out


class DeviceRun(dc.DeviceRun):
    """defrag_cases.DeviceRun through pcppx_defrag6_device."""

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.defrag6_device(self.data, self.offsets, self.caplens, c.n, 1, self.layers, ML, self.info, _spec(c),
                              self.d_off, self.d_cap, self.d_tot, c.maxp(), self.d_data, c.cap(), self.d_idx,
                              self.d_first, self.d_frags, self.d_disp, stream, data_len=self.data_len,
                              summary=self.summary, brief=self.brief)


def run_device(engine, c: Case, device: str = "cuda:0", source=None) -> Buffers:
    import torch

    run = DeviceRun(c, device, source)
    run.launch(engine, torch.cuda.current_stream(device).cuda_stream)
    return run.result()


# ------------------------------------------------------------------ packets
def addr6(k: int) -> bytes:
    return bytes.fromhex("20010db8") + bytes(8) + struct.pack(">I", k)


def ipv6(src: int, dst: int, nh: int, body: bytes, plen: int | None = None) -> bytes:
    """The fixed header and what follows it (extensions and payload)."""
    return struct.pack(">IHBB", 0x60000000, len(body) if plen is None else plen, nh, 64) + addr6(src) + addr6(dst) + body


def frag_hdr(nh: int, foff: int, more: bool, ident: int) -> bytes:
    assert foff % 8 == 0
    return struct.pack(">BBHI", nh, 0, foff | (1 if more else 0), ident)


def opts_hdr(nh: int, units: int = 1) -> bytes:
    """A Hop-by-Hop or Destination-Options header of units * 8 bytes: one PadN option."""
    return bytes([nh, units - 1, 1, units * 8 - 4]) + bytes(units * 8 - 4)


def group6(rng, ident: int, sizes: list[int], src: int = 1, dst: int = 2, vlan: int | None = None, ahead: int = 0,
           behind: int = 0, trailer: bytes = b"", proto: int = 17, datagram: bytes | None = None) -> list[bytes]:
    """The fragments of one UDP datagram over IPv6, in offset order. ahead: 8-byte units of a Hop-by-Hop header in
    front of the fragment header; behind: units of a Destination-Options header behind it, in every fragment (a
    crafted shape: parseExtensions walks on behind the fragment header, so every member's hdr includes it). The first
    fragment may carry a trailer."""
    l2 = dc.eth(vlan, 0x86DD)
    d = dc.udp_datagram(rng, sum(sizes)) if datagram is None else datagram
    pk = []
    for off, piece, more in dc.split(d, sizes):
        ext = (opts_hdr(44, ahead) if ahead else b"") + frag_hdr(60 if behind else proto, off, more, ident)
        ext += opts_hdr(proto, behind) if behind else b""
        p = l2 + ipv6(src, dst, 0 if ahead else 44, ext + piece)
        pk.append(p + (trailer if off == 0 else b""))
    return pk


def filler6(rng, k: int) -> bytes:
    """A small unfragmented UDP packet over IPv6."""
    return dc.eth(ethertype=0x86DD) + ipv6(0x100 + k % 251, 0x200 + k % 241, 17, dc.udp_datagram(rng, 8 + k % 19))


def fragment_rows(c: Case) -> np.ndarray:
    return c.info["ip_status"] & 15 == abi.IPR_FRAGMENT


def output_totals(c: Case):
    t = brute(replace(c, data_cap=None, max_packets=None, max_fragments=0, index_only=True)).totals
    return int(t[abi.DEFRAG_OUT_PACKETS]), int(t[abi.DEFRAG_OUT_BYTES]), int(t[abi.DEFRAG_CANDIDATES])


# ------------------------------------------------------------------ the families
CLEAN = []    # names of the cases all of whose fragment groups are clean: every candidate must be merged
UNCLEAN = []  # names of the cases whose crafted group must stay LEFT (a clean group beside it is reassembled)
EXPECT = {}   # name -> (reassembled, left) where the case states its result outright


def _clean(c: Case) -> Case:
    CLEAN.append(c.name)
    return c


def _unclean(c: Case) -> Case:
    UNCLEAN.append(c.name)
    return c


def quirk_cases(rng=None) -> list[Case]:
    """The crafted shapes whose reassembled bytes tests/golden/defrag6/expected.npz records from the reference."""
    rng = np.random.default_rng(66) if rng is None else rng
    out = []
    out.append(make("swap_0600", group6(rng, 0x600, [496, 496, 496])))          # T + H = 1488 + 48 = 0x0600: field 6
    out.append(make("swap_0800", group6(rng, 0x800, [1000, 1000])))             # 2000 + 48 = 0x0800: field 8
    out.append(make("swap_04d8", group6(rng, 0x4D8, [496, 496, 200])))          # 1192 + 48: 0xD804 > T, field 1192
    out.append(make("hbh_ahead_0600", group6(rng, 0x601, [496, 496, 488], ahead=1)))  # 1480 + 56 = 0x0600, E = 16
    out.append(make("hbh_ahead", group6(rng, 0x602, [16, 24, 11], ahead=1)[::-1]))
    out.append(make("dst_behind", group6(rng, 0x603, [24, 8, 13], ahead=1, behind=1)))  # E = 24
    out.append(make("vlan_shuffled", [group6(rng, 0x604, [8, 16, 24, 9], vlan=7)[j] for j in (2, 0, 3, 1)]))
    # a trailer: the layer is clamped to payloadLength + hdr, which counts the E extension bytes twice, so E bytes of a
    # trailer count as payload. 20 trailer bytes behind 16: the first member's len is 24, the next one sits at 24, the
    # other 12 trailer bytes are dropped
    g = group6(rng, 0x605, [24, 16, 5])
    first = bytearray(g[0][:-8] + bytes(range(0xE0, 0xF4)))
    first[14 + 4:14 + 6] = struct.pack(">H", 8 + 16)
    out.append(make("trailer_long", [bytes(first), g[1], g[2]]))
    # 6 trailer bytes behind 16: len 22, the next member at 16 lies below currentOffset: the duplicate path, LEFT
    g = group6(rng, 0x606, [16, 16, 5], trailer=bytes(range(0xD0, 0xD6)))
    out.append(make("trailer_short", g))
    return out


QUIRK_LEFT = ("trailer_short",)


def cases() -> list[Case]:
    CLEAN.clear()
    UNCLEAN.clear()
    EXPECT.clear()
    out: list[Case] = []
    rng = np.random.default_rng(2026)
    # group sizes, in order, reversed and shuffled, alone in the batch
    for k in (2, 3, 64):
        g = group6(rng, 0x100 + k, dc.sizes_for(k, rng))
        out.append(_clean(make(f"g{k}_in_order", g)))
        out.append(_clean(make(f"g{k}_reversed", g[::-1], passthrough=k != 3)))
        out.append(_clean(make(f"g{k}_shuffled", [g[int(j)] for j in rng.permutation(k)])))
    g = group6(rng, 0x165, dc.sizes_for(65, rng))
    out.append(_unclean(make("g65_too_many", [g[int(j)] for j in rng.permutation(65)])))
    EXPECT["g65_too_many"] = (0, 65)
    # the recorded quirk shapes: extensions ahead and behind, VLAN, the byte-swap clamp, trailers
    for c in quirk_cases():
        out.append(_unclean(c) if c.name in QUIRK_LEFT else _clean(c))
    # every destination residue: groups of payloads 8 / 16 / 24 / 1232 behind fillers whose lengths step by one byte,
    # so that the packet's start (the first member's first piece) and its payload pieces meet all 16 residues
    pk = []
    for j in range(96):
        pk.append(dc.eth() + dc.ipv4(0x0A010000 + j, 0x0A020000, j, dc.udp_datagram(rng, 8 + j % 16 + (j // 16))))
        pk += group6(rng, 0x2000 + j, [(8, 16, 24, 1232)[j % 4], (1232, 24, 16, 8)[j % 4], 5 + j % 7], src=0x300 + j,
                     ahead=int(j % 3 == 1), vlan=5 if j % 5 == 0 else None)
    out.append(_clean(replace(make("residues", pk), out_misalign=3, src_misalign=7)))
    # both families interleaved, groups across the block edge; the three specs over the same packets
    v4 = [dc.group(rng, 0x3000 + j, dc.sizes_for(2 + j % 4, rng), src=0x0A000100 + j) for j in range(40)]
    v6 = [group6(rng, 0x4000 + j, dc.sizes_for(2 + j % 5, rng), src=0x500 + j, ahead=j % 2) for j in range(40)]
    mixed = dc.spread(rng, v4 + v6, BLOCK + 1, extra={9: filler6(rng, 9), BLOCK - 1: filler6(rng, 3)})
    n4, n6 = sum(len(g) for g in v4), sum(len(g) for g in v6)
    for fam, name, exp in ((V4 | V6, "interleaved", (80, 0)), (V6, "interleaved_v6", (40, n4)),
                           (V4, "interleaved_v4", (40, n6))):
        c = make(name, mixed, families=fam)
        EXPECT[name] = exp
        out.append(_clean(c) if fam == V4 | V6 else c)
    out.append(_clean(replace(make("interleaved_brief", mixed, passthrough=False), use_brief=True, out_misalign=11)))
    # the unclean families: one crafted group, and a clean one beside it that must still be reassembled
    ok = group6(rng, 0x400, [16, 16, 9], src=7)

    def crafted(name: str, frs: list[bytes], **kw) -> Case:
        c = _unclean(make(name, dc.spread(rng, [frs, ok], len(frs) + len(ok) + 9), **kw))
        EXPECT[name] = (1, len(frs))
        out.append(c)
        return c

    d = dc.udp_datagram(rng, 48)
    fr = lambda off, piece, more, ident: dc.eth(ethertype=0x86DD) + ipv6(1, 2, 44, frag_hdr(17, off, more, ident) + piece)  # noqa
    crafted("gap", [fr(0, d[:16], True, 0x410), fr(24, d[24:], False, 0x410)])
    crafted("overlap", [fr(0, d[:24], True, 0x411), fr(16, d[16:], False, 0x411)])
    crafted("duplicate_first", [fr(0, d[:16], True, 0x412), fr(0, d[:16], True, 0x412), fr(16, d[16:], False, 0x412)])
    crafted("no_last", [fr(0, d[:16], True, 0x415), fr(16, d[16:32], True, 0x415), fr(32, d[32:], True, 0x415)])
    crafted("two_last", [fr(0, d[:16], True, 0x414), fr(16, d[16:32], False, 0x414), fr(32, d[32:], False, 0x414)])
    # records that describe a chain the bytes do not hold: the first member's hdr 8 bytes longer (the tiling kept exact
    # by moving the other members down), so the walk ends short of hdr
    bad = group6(rng, 0x416, [24, 16, 5])
    c = crafted("chain_short_of_hdr", bad)
    rows = [i for i in np.nonzero(fragment_rows(c))[0] if int(c.info["frag_id"][i]) == 0x416]
    assert len(rows) == 3
    for i in rows:
        if int(c.info["frag_offset"][i]) == 0:
            k = [int(p) for p in c.layers[i]["proto"]].index(P_IPV6)
            c.layers[i, k]["hdr_len"] += 8
        else:
            c.info["frag_offset"][i] -= 8
    # a chain that goes on behind hdr: the fragment header names a Destination-Options header that the records do not
    # count (the fragment is too short for the parse to walk it; the reassembled packet is not)
    bad = [dc.eth(ethertype=0x86DD) + ipv6(1, 2, 44, frag_hdr(nh, off, more, 0x417) + piece)
           for nh, off, piece, more in ((60, 0, b"\x11", True), (17, 8, d[:16], False))]
    c = crafted("chain_goes_on", bad)
    rows = [i for i in np.nonzero(fragment_rows(c))[0] if int(c.info["frag_id"][i]) == 0x417]
    c.info["frag_offset"][rows[1]] = 1  # tile behind the one-byte first member
    # the size bounds. ip_off + hdr + total <= PCPPX_MAX_CAPLEN is the tighter one behind an Ethernet header
    # (14 + 48 + 65473 = 65535), so hdr + total = 65535 cannot be reached; both are in the models
    for name, total, good in (("total_65473", 65473, True), ("total_65474", 65474, False)):
        sz = [total // 2 // 8 * 8]
        sz.append(total - sz[0])
        c = make(name, dc.spread(rng, [group6(rng, 0x420, sz)], 5))
        EXPECT[name] = (1, 0) if good else (0, 2)
        out.append(_clean(c) if good else _unclean(c))
    # two families under one key (info is an input column). families = V4: the IPv6 fragments stay outside the table and
    # the IPv4 group is reassembled, as pcppx_defrag_device does; V6 and V4 | V6: one mixed group, everything LEFT
    a, b = dc.group(rng, 0x440, [16, 7]), group6(rng, 0x441, [16, 16, 3])
    pk = dc.spread(rng, [a, b], 12)
    for fam, exp in ((V4, (1, 3)), (V6, (0, 5)), (V4 | V6, (0, 5))):
        c = make(f"families_share_a_key_f{fam}", pk, families=fam)
        c.info["ip_key"][fragment_rows(c)] = 0xDEADBEEF
        EXPECT[c.name] = exp
        out.append(c)
    # a family the spec does not ask for, under keys of its own: LEFT, and the other family is reassembled
    pk = dc.spread(rng, [a, b], 12)
    for fam, exp in ((V4, (1, 3)), (V6, (1, 2))):
        c = make(f"unasked_family_f{fam}", pk, families=fam)
        EXPECT[c.name] = exp
        out.append(c)
    # bad descriptors; descriptors in another order than the bytes
    for pt in (True, False):
        out.append(mc.with_bad_descriptors(make(f"bad_desc_pt{int(pt)}", dc.spread(rng, v4[:10] + v6[:15], 400),
                                                passthrough=pt)))
    c = make("shuffled_descriptors", dc.spread(rng, v6[:20], 300))
    out.append(_clean(dc.permuted(c, rng.permutation(c.n))))
    # capacities: exact and one short; index-only; no optional columns
    base = make("cap", dc.spread(rng, v6[:25] + v4[:5], 500))
    op, ob, nc = output_totals(base)
    for nm, kw in (("cap_exact", dict(data_cap=ob, max_packets=op, max_fragments=nc)), ("cap_short1", dict(data_cap=ob - 1)),
                   ("maxp_short1", dict(max_packets=op - 1)), ("maxf_short1", dict(max_fragments=nc - 1)),
                   ("index_only", dict(index_only=True)), ("index_only_maxp_short1", dict(index_only=True, max_packets=op - 1)),
                   ("no_columns", dict(want_index=False, want_columns=False)),
                   ("only_reassembled", dict(passthrough=False)),
                   ("only_reassembled_short1", dict(passthrough=False, max_packets=29))):
        out.append(replace(base, name=nm, **kw))
    out.append(make("n0", []))
    out.append(make("n1_fragment", [ok[0]]))
    out.append(make("no_candidates", [filler6(rng, k) for k in range(130)], passthrough=False))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


OVERFLOWING = ("cap_short1", "maxp_short1", "maxf_short1", "index_only_maxp_short1", "only_reassembled_short1")
