"""pcppx_defrag6_device: the IPv4 and IPv6 fragment groups that are complete inside one device batch (include/pcppx.h,
defrag6).

CPU: the ctypes mirror matches the header, both symbols are exported and every bad-argument combination is refused
before any device work; pcppx_defrag6_reference equals a brute-force Python restatement of the contract on every case
of tests/defrag6_cases.py, whole buffers and fill included; with families = V4 it equals pcppx_defrag_reference on the
IPv4 cases of tests/defrag_cases.py; the streaming model of processPacket with the IPv6 finish reproduces the
reference's own vectors for ip6_fragments.pcap (tests/golden/defrag6) in capture order and shuffled, and so does the
reference function; the crafted quirk shapes (byte-swapped payload length, extensions ahead of and behind the fragment
header, trailers) give the bytes recorded from the reference (expected.npz).
GPU: pcppx_defrag6_device equals pcppx_defrag6_reference byte for byte on every case; families = V4 is bit-identical to
pcppx_defrag_device; two streams and a repeat agree; fragment6 / fragment -> parse + reasm -> defrag6 -> parse gives the
unfragmented batch back; an IPv6 case with its source on both sides of offset 2^32.
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import defrag6_cases as d6
import defrag_cases as dc
import oracle
from conftest import GOLDEN
from pcapplusplus_amd import abi, frag
from pcapplusplus_amd.pcap import PacketBatch, from_packets, read_hex_dat, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "defrag6"
CAPTURE = GOLDEN / "ingest" / "files" / "Tests__Pcap++Test__PcapExamples__ip6_fragments.pcap"
CASES = d6.cases()
BY_NAME = {c.name: c for c in CASES}
V4_CASES = [c for c in dc.cases() if c.n <= 3200]
V4, V6 = d6.V4, d6.V6


# ---------------------------------------------------------------- CPU: the ABI
def test_defrag6_struct_matches_header():
    fields = [f for f, _ in abi.Defrag6Spec._fields_]
    lines = "".join(f'  printf("{f} %zu %zu\\n", offsetof(pcppx_defrag6_spec, {f}), '
                    f'sizeof(((pcppx_defrag6_spec*)0)->{f}));\n' for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %d %d %d\\n", sizeof(pcppx_defrag6_spec), PCPPX_DEFRAG_FAM_V4, PCPPX_DEFRAG_FAM_V6, '
           'PCPPX_ABI_VERSION);\n' + lines + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.Defrag6Spec), abi.DEFRAG_FAM_V4, abi.DEFRAG_FAM_V6, 7]
    assert C.sizeof(abi.Defrag6Spec) == C.sizeof(abi.DefragSpec) == 8
    assert len(out) == 1 + len(fields)
    for line in out[1:]:
        name, off, size = line.split()
        d = getattr(abi.Defrag6Spec, name)
        assert (d.offset, d.size) == (int(off), int(size)), name
    s = abi.make_defrag6_spec(False, 9, V6)
    assert (s.max_fragments, s.passthrough, s.families, list(s.reserved)) == (9, 0, 2, [0, 0])


def test_defrag6_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_defrag6_device", "pcppx_defrag6_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_defrag6_spec(True, 0, V4 | V6)
    o = abi.Defragged(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, info=1, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _spec_reserved(a, k):
    a["s"].reserved[k] = 1


BAD_ARGS = {
    "families_0": lambda a: _set(a, "s", "families", 0),
    "families_4": lambda a: _set(a, "s", "families", 4),
    "families_7": lambda a: _set(a, "s", "families", 7),
    "families_255": lambda a: _set(a, "s", "families", 255),
    "spec_reserved_0": lambda a: _spec_reserved(a, 0),
    "spec_reserved_1": lambda a: _spec_reserved(a, 1),
    "passthrough_2": lambda a: _set(a, "s", "passthrough", 2),
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_offsets": lambda a: _set(a, "o", "offsets", None),
    "null_caplens": lambda a: _set(a, "o", "caplens", None),
    "null_info": lambda a: a.update(info=None),
    "null_layers": lambda a: _set(a, "r", "layers", None),
    "null_summary_and_brief": lambda a: _set(a, "r", "summary", None),
    "null_batch_offsets": lambda a: _set(a, "b", "offsets", None),
    "null_batch_caplens": lambda a: _set(a, "b", "caplens", None),
    "null_batch_data": lambda a: _set(a, "b", "data", None),
    "packed_records": lambda a: _set(a, "r", "layout", abi.LAYOUT_PACKED),
    "dense_records": lambda a: _set(a, "r", "layout", abi.LAYOUT_DENSE),
    "max_layers_0": lambda a: a.update(ml=0),
    "max_layers_17": lambda a: a.update(ml=17),
    "out_reserved": lambda a: _set(a, "o", "reserved", 1),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_defrag6_device(ctx, ref("b"), ref("r"), a["ml"], a["info"], ref("s"), ref("o"), None)
    host = None if ctx is None else \
        lib.pcppx_defrag6_reference(ref("b"), ref("r"), a["ml"], a["info"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_defrag6_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_defrag6_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    for fam in (V4, V6, V4 | V6):  # every legal families value passes the checks; n == 0 gives zero totals
        empty = d6.run_reference(replace(BY_NAME["n0"], families=fam))
        assert list(empty.totals) == [0] * abi.DEFRAG_TOTALS
        d6.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    want = d6.brute(case)
    got = d6.run_reference(case)
    d6.assert_same(got, want, case.name)
    t = abi.defrag_totals_dict(got.totals)
    if case.name in d6.OVERFLOWING:
        assert t["overflow"] == 1
        d6.assert_untouched(got, case.name)
    if case.name in d6.CLEAN:  # a runner that leaves everything LEFT cannot pass
        assert t["reassembled"] > 0 and t["merged_frags"] == t["candidates"] and t["left_frags"] == 0
    if case.name in d6.UNCLEAN:
        assert t["left_frags"] > 0
    if case.name in d6.EXPECT:
        assert (t["reassembled"], t["left_frags"]) == d6.EXPECT[case.name], case.name


@pytest.mark.parametrize("case", V4_CASES, ids=lambda c: c.name)
def test_families_v4_equals_defrag_reference(case):
    """Every column and byte, on the IPv4 cases of defrag_cases (IPv6 fragments among them); and asking for both
    families changes nothing where no IPv6 group is complete."""
    want = dc.run_reference(case)
    d6.assert_same(d6.run_reference(d6.widen(case, V4)), want, case.name)
    if case.name != "mixed":  # its two IPv6 fragments become candidates there
        d6.assert_same(d6.run_reference(d6.widen(case, V4 | V6)), want, case.name)


def test_cases_cover_the_kernel_shapes():
    sizes = set()
    for c in CASES:
        rows = d6.fragment_rows(c) & ((c.info["ip_status"] & abi.IPR_F_IPV6) != 0)
        sizes |= {int(x) for x in np.unique(c.info["ip_key"][rows], return_counts=True)[1]}
    assert {2, 3, 64, 65} <= sizes
    # the header lengths (E = 8, 16, 24) and both link headers among the first members of reassembled IPv6 groups
    seen = set()
    for name in d6.CLEAN:
        c = BY_NAME[name]
        got = d6.brute(replace(c, want_columns=True, want_index=True))
        for j in np.nonzero(got.frags[:int(got.totals[abi.DEFRAG_OUT_PACKETS])])[0]:
            f = int(got.first[j])
            if int(c.info["ip_status"][f]) & abi.IPR_F_IPV6:
                k = [int(p) for p in c.layers[f]["proto"]].index(d6.P_IPV6)
                seen.add((int(c.layers[f, k]["offset"]), int(c.layers[f, k]["hdr_len"])))
    assert {(14, 48), (14, 56), (14, 64), (18, 48), (18, 56)} <= seen, seen
    # every (destination mod 16) for the reassembled packet's start (the first member's first piece) and for payload
    # pieces of 8, 16, 24 and 1232 bytes
    c = BY_NAME["residues"]
    got = d6.brute(c)
    kinds = d6.candidates(c)
    starts, first_payload, others, lens = set(), set(), set(), set()
    for j in np.nonzero(got.frags[:int(got.totals[abi.DEFRAG_OUT_PACKETS])])[0]:
        pos = int(got.offsets[j]) + c.out_misalign
        starts.add(pos % 16)
        f = int(got.first[j])
        for i in np.nonzero(c.info["ip_key"] == c.info["ip_key"][f])[0]:
            ln = kinds[int(i)][1][2]
            at = (pos + kinds[f][1][0] + 40 + int(c.info["frag_offset"][i])) % 16
            (first_payload if int(i) == f else others).add(at)
            lens.add(ln)
    assert starts == first_payload == others == set(range(16)) and {8, 16, 24, 1232} <= lens
    t = abi.defrag_totals_dict(d6.brute(BY_NAME["interleaved"]).totals)
    assert BY_NAME["interleaved"].n == d6.BLOCK + 1 and t["reassembled"] == 80
    # the clamp: the payload-length field of the three byte-swap shapes
    for name, field in (("swap_0600", 6), ("swap_0800", 8), ("swap_04d8", 1192), ("hbh_ahead_0600", 6)):
        (_, _, pkt), = d6.reassembled(d6.brute(BY_NAME[name]))
        assert int.from_bytes(pkt[18:20], "big") == field and pkt[20] == 17
        assert len(pkt) - 54 == {"swap_0600": 1488, "swap_0800": 2000, "swap_04d8": 1192, "hbh_ahead_0600": 1480}[name]


# ---------------------------------------------------------------- CPU: the reference's own vectors and the recorded ones
def parsed_case(batch: PacketBatch, name: str, **kw) -> d6.Case:
    summary, layers = oracle.oracle_parse(batch, dc.OPTS)
    info = oracle.oracle_reasm(batch, summary, layers)
    return d6.Case(name, batch.data[:int(batch.caplens.sum())], batch.offsets, batch.caplens, summary=summary,
                   layers=layers, info=info, **kw)


def _vector_groups(c: d6.Case):
    """The capture's two fragment ids, in the order the reference's test names them (packet1: the first to appear)."""
    ids = c.info["frag_id"][d6.fragment_rows(c)]
    _, firsts = np.unique(ids, return_index=True)
    return [int(ids[k]) for k in sorted(firsts)]


def test_stream_model_and_reference_reproduce_the_ip6_vectors():
    c = parsed_case(read_pcap(CAPTURE), "ip6_fragments.pcap")
    assert bool(((c.info["ip_status"][d6.fragment_rows(c)] & abi.IPR_F_IPV6) != 0).all())
    ids = _vector_groups(c)
    want = {ids[0]: read_hex_dat(VECTORS / "ip6_fragments_packet1.txt"),
            ids[1]: read_hex_dat(VECTORS / "ip6_fragments_packet2.txt")}
    orders = [np.arange(c.n)] + [np.random.default_rng(s).permutation(c.n) for s in range(5)]
    for perm in orders:
        p = dc.permuted(c, perm)
        st = d6.stream(p)
        got = d6.run_reference(p)
        packets = d6.reassembled(got)
        by_id = {int(p.info["frag_id"][f]): pkt for _, f, pkt in packets}
        for ident in ids[:2]:  # packets 1 and 2 of the reference's test
            # the vectors carry a payload length of 737 / 1448, which the reference's own test writes into the result
            # before it compares ("small fix for payload length which is wrong in the original packet",
            # IPFragmentationTests.cpp:121, 805, 812); the library's value is the clamp rule's, here T = 741 / 1452
            pkt, vec = by_id[ident], want[ident]
            assert len(pkt) == len(vec) and int.from_bytes(pkt[18:20], "big") == len(pkt) - 54
            assert int.from_bytes(vec[18:20], "big") == len(vec) - 54 - 4
            assert pkt[:18] + vec[18:20] + pkt[20:] == vec
        for i, f, pkt in packets:  # where the reference returns them, and what
            assert st[i] == (pkt, f)
        assert sorted(st) == sorted(i for i, _, _ in packets)
    # families = V4: nothing happens to them
    got = d6.run_reference(replace(c, families=V4))
    assert int(got.totals[abi.DEFRAG_REASSEMBLED]) == 0
    assert int(got.totals[abi.DEFRAG_LEFT_FRAGS]) == int(d6.fragment_rows(c).sum())


def test_recorded_quirk_vectors_match_the_reference_function():
    rec = np.load(VECTORS / "expected.npz")
    for case in d6.quirk_cases():
        name = case.name
        lens = rec[f"{name}.lens"]
        ends = np.cumsum(lens)
        pk = [rec[f"{name}.packets"][e - n:e].tobytes() for e, n in zip(ends, lens)]
        assert pk == [case.batch().packet(i) for i in range(case.n)], name  # the inputs the recording was made from
        c = parsed_case(from_packets(pk), name)
        packets = d6.reassembled(d6.run_reference(c))
        at = int(rec[f"{name}.at"][0])
        if at < 0:
            assert packets == [] and name in d6.QUIRK_LEFT, name
            assert d6.stream(c) == {}
            continue
        (i, f, pkt), = packets
        assert i == at and pkt == rec[f"{name}.out"].tobytes(), name
        assert d6.stream(c) == {at: (pkt, f)}, name


# (the stream holds both families, so a spec that leaves the IPv6 fragments outside the table, as pcppx_defrag_device
# does, is not comparable where the families share a key)
SMALL = [c for c in CASES if c.n <= 1100 and c.families != V4]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_reassembled_packets_are_what_the_stream_returns(case):
    """In source order and in three seeded permutations: every packet the contract reassembles equals, byte for byte
    and at the same position, what processPacket returns for that order of arrival."""
    if not case.want_columns or case.index_only or case.name in d6.OVERFLOWING:
        case = replace(case, want_columns=True, want_index=True, index_only=False, data_cap=None, max_packets=None,
                       max_fragments=0)
    orders = [np.arange(case.n)] + [np.random.default_rng(100 + s).permutation(case.n) for s in range(3)]
    for perm in orders:
        c = dc.permuted(case, perm)
        got = d6.run_reference(c)
        st = d6.stream(c)
        packets = d6.reassembled(got)
        assert len(packets) == int(got.totals[abi.DEFRAG_REASSEMBLED])
        for i, f, pkt in packets:
            assert i in st and st[i] == (pkt, f), (case.name, i)
        if case.name in d6.CLEAN:
            assert sorted(st) == sorted(i for i, _, _ in packets)  # and the stream returns nothing else


# ---------------------------------------------------------------- CPU: the fragmenter
def _mixed_batch(n: int, seed: int) -> PacketBatch:
    """IPv4 and IPv6 UDP / TCP packets, some behind a VLAN tag, some IPv6 ones behind a Hop-by-Hop header."""
    rng = np.random.default_rng(seed)
    pk = []
    for k in range(n):
        size = int(rng.choice([8, 30, 64, 65, 200, 1000, 1440, 1488]))
        udp = k % 3 != 0
        l4 = dc.udp_datagram(rng, size, 1024 + k % 50, 2000 + k % 7) if udp else \
            dc.struct.pack(">HHIIBBHHH", 1024 + k % 9000, 80, k, 0, 0x50, 0x10, 512, 0, 0) + \
            bytes(rng.integers(0, 256, max(size - 8, 0), dtype=np.uint8))
        proto = 17 if udp else 6
        vlan = 7 if k % 4 == 0 else None
        if k % 2:
            body = (d6.opts_hdr(proto) if k % 5 == 0 else b"") + l4
            pk.append(dc.eth(vlan, 0x86DD) + d6.ipv6(0x1000 + k % 97, 0x2000 + k % 89, 0 if k % 5 == 0 else proto, body))
        else:
            pk.append(dc.eth(vlan) + dc.ipv4(0x0A000000 + k % 97, 0x0B000000 + k % 89, k & 0xFFFF, l4, proto=proto))
    pk[3] = dc.eth(ethertype=0x0806) + bytes(28)
    return from_packets(pk)


def test_fragmenter6_follows_ipfragutil():
    base = _mixed_batch(200, 3)
    ids = (np.arange(base.n) * 2654435761 % (1 << 32)).astype(np.uint32)
    out = frag.fragment6(base, 60, ids)  # rounded down to 56
    src, no, cnt = out.meta["frag_src"], out.meta["frag_no"], out.meta["frag_count"]
    v6, ip_off, hdr, pay, nh_at, fragmented = frag.locate_ipv6(base)
    assert int(v6.sum()) == 99 and not fragmented.any() and set(hdr[v6]) == {40, 48}
    summary, layers = oracle.oracle_parse(out, dc.OPTS)
    info = oracle.oracle_reasm(out, summary, layers)
    for i in range(base.n):
        rows = np.nonzero(src == i)[0]
        if not v6[i] or pay[i] <= 56:
            assert len(rows) == 1 and out.packet(int(rows[0])) == base.packet(i)
            continue
        assert len(rows) == -(-int(pay[i]) // 56) == int(cnt[rows[0]]) and list(no[rows]) == list(range(len(rows)))
        p = base.packet(i)
        o, h, at = int(ip_off[i]), int(hdr[i]), int(nh_at[i])
        body = b""
        for k, r in enumerate(rows):
            q = out.packet(int(r))
            same = bytearray(q[:o + h])
            same[o + 4:o + 6] = p[o + 4:o + 6]
            same[at] = p[at]
            assert bytes(same) == p[:o + h] and q[at] == 44
            assert int.from_bytes(q[o + 4:o + 6], "big") == len(q) - o - 40
            fh = q[o + h:o + h + 8]
            assert fh[0] == p[at] and fh[1] == 0 and int.from_bytes(fh[4:], "big") == int(ids[i])
            assert int.from_bytes(fh[2:4], "big") == (k * 56) | (1 if k + 1 < len(rows) else 0)
            st = int(info["ip_status"][r])
            assert st & 15 == abi.IPR_FRAGMENT and st & abi.IPR_F_IPV6 and int(info["frag_offset"][r]) == k * 56
            assert bool(st & abi.IPR_F_LAST) == (k + 1 == len(rows)) and int(info["frag_id"][r]) == int(ids[i])
            k6 = [int(x) for x in layers[r]["proto"]].index(d6.P_IPV6)
            assert int(layers[r, k6]["hdr_len"]) == h + 8
            body += q[o + h + 8:]
        assert body == p[o + h:o + h + int(pay[i])]
    assert list(frag.locate_ipv6(out)[5]) == list(cnt > 1)
    again = frag.fragment6(out, 8, np.zeros(out.n, np.uint32))  # a fragment is not fragmented again
    was = np.isin(again.meta["frag_src"], np.nonzero(cnt > 1)[0])
    assert was.any() and (again.meta["frag_count"][was] == 1).all() and again.n > out.n
    only = frag.fragment6(base, 56, ids, select=np.arange(base.n) % 4 == 1)
    assert set(only.meta["frag_src"][only.meta["frag_count"] > 1] % 4) == {1}
    with pytest.raises(ValueError):
        frag.fragment6(base, 7, ids)
    with pytest.raises(ValueError):
        frag.fragment6(base, 56, ids[:-1])


def _expected_round_trip(base: PacketBatch, fr: PacketBatch, frags) -> list[bytes]:
    """The unfragmented packets as the reference gives them back: an IPv4 one with DF cleared and its checksum
    recomputed; an IPv6 one unchanged but for the payload-length clamp."""
    v6, ip_off, hdr, pay, nh_at, _ = frag.locate_ipv6(base)
    pk = []
    for j in range(base.n):
        p = bytearray(base.packet(j))
        if frags[j] and v6[j]:
            o, t, h = int(ip_off[j]), int(pay[j]), int(hdr[j])
            nh = p[int(nh_at[j])]
            del p[o + 40:o + h]  # the extensions ahead of the fragment header are cut as well
            p = bytearray(d6.patched6(p, o, h + 8, t, nh))
        elif frags[j]:
            o = 18 if p[12:14] == b"\x81\x00" else 14
            p = bytearray(dc.patched(p, o, 20, len(p) - o - 20))
        pk.append(bytes(p))
    return pk


def test_fragment_both_families_then_reference_gives_the_datagrams_back():
    base = _mixed_batch(300, 4)
    ids = np.arange(base.n, dtype=np.uint32) + 77
    fr = frag.fragment(base, 576)
    fr = frag.fragment6(fr, 576, ids[fr.meta["frag_src"]])
    c = parsed_case(fr, "round_trip")
    got = d6.run_reference(c)
    t = abi.defrag_totals_dict(got.totals)
    assert t["out_packets"] == base.n and t["left_frags"] == 0 and t["merged_frags"] == t["candidates"] > 100
    out = PacketBatch(got.data, got.offsets[:base.n], got.caplens[:base.n])
    want = _expected_round_trip(base, fr, got.frags[:base.n])
    v6 = frag.locate_ipv6(base)[0]
    assert int((got.frags[:base.n][v6] != 0).sum()) > 20 and int((got.frags[:base.n][~v6] != 0).sum()) > 20
    for j in range(base.n):
        assert out.packet(j) == want[j], j


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_defrag6_equals_reference(engine, case):
    want = d6.run_reference(case)
    got = d6.run_device(engine, case)
    d6.assert_same(got, want, case.name)
    if case.name in d6.OVERFLOWING:
        d6.assert_untouched(got, case.name)
    if case.name in d6.CLEAN:
        assert int(got.totals[abi.DEFRAG_REASSEMBLED]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "many_groups_brief", "bad_desc_pt1"])
def test_gpu_families_v4_is_bit_identical_to_defrag_device(engine, name):
    case = next(c for c in V4_CASES if c.name == name)
    want = dc.run_device(engine, case)
    got = d6.run_device(engine, d6.widen(case, V4))
    d6.assert_same(got, want, name)
    d6.assert_same(got, dc.run_reference(case), name)
    c6 = replace(BY_NAME["interleaved_v4"])  # and on a batch that holds complete IPv6 groups
    as_v4 = dc.Case(**{f: getattr(c6, f) for f in dc.Case.__dataclass_fields__})
    d6.assert_same(d6.run_device(engine, c6), dc.run_device(engine, as_v4), "interleaved_v4")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["interleaved", "g64_shuffled", "residues"])
def test_gpu_defrag6_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = d6.run_reference(case)
    runs = [d6.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        d6.assert_same(r.result(), want, f"{name} run {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 9])
def test_gpu_defrag6_source_on_both_sides_of_4gib(engine, mis):
    """test_gpu_defrag_source_on_both_sides_of_4gib for a batch of both families: the packets laid around offset 2^32
    and around the offset whose address is a multiple of 2^32, members of one IPv6 group on both sides."""
    import torch

    import wide_cases as wc

    case = replace(BY_NAME["interleaved_brief"], src_misalign=0, out_misalign=3)
    raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device="cuda:0")
    lay = wc.layout(raw.data_ptr(), mis)
    data = raw[lay.pad: lay.pad + lay.data_len]
    n, half = case.n, case.n // 2
    lens = case.caplens.astype(np.int64)
    offs = np.zeros(n, np.int64)
    for lo, hi, line in ((0, half, lay.lines[0]), (half, n, lay.lines[1])):
        run = np.cumsum(lens[lo:hi]) - lens[lo:hi]
        mid = (lo + hi) // 2 - lo
        start = line - int(run[mid]) - int(lens[lo + mid]) // 2  # packet `mid` of the run lies across the line
        offs[lo:hi] = start + run
        k = lo + mid
        assert offs[k] < line < offs[k] + lens[k]
        src0 = int(case.offsets[lo])
        chunk = case.data[src0:src0 + int(lens[lo:hi].sum())]
        data[start:start + len(chunk)] = torch.from_numpy(chunk).to("cuda:0")
    order = np.random.default_rng(5).permutation(n)  # descriptors of both sides interleaved
    wide = dc.permuted(replace(case, offsets=offs.astype(np.uint64)), order)
    compact = dc.permuted(case, order)
    source = (data, torch.from_numpy(wide.offsets.view(np.int64)).to("cuda:0"),
              torch.from_numpy(wide.caplens.view(np.int32)).to("cuda:0"), lay.data_len)
    want = d6.run_reference(compact)
    assert int(want.totals[abi.DEFRAG_REASSEMBLED]) == 80
    rows6 = d6.fragment_rows(compact) & ((compact.info["ip_status"] & abi.IPR_F_IPV6) != 0)
    sides = [{bool(wide.offsets[j] < wc.LINE) for j in np.nonzero(compact.info["ip_key"] == k)[0]}
             for k in np.unique(compact.info["ip_key"][rows6])]
    assert any(len(s) == 2 for s in sides)
    got = d6.run_device(engine, compact, source=source)
    d6.assert_same(got, want, f"wide mis{mis}")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_fragment_parse_defrag6_parse_end_to_end(engine):
    from pcapplusplus_amd.engine import defrag6_on_device, parse_on_device
    from test_defrag import _device_parse_reasm

    base = _mixed_batch(1500, 6)
    ids = np.arange(base.n, dtype=np.uint32) * 3 + 1
    fr = frag.fragment(base, 576)
    fr = frag.fragment6(fr, 576, ids[fr.meta["frag_src"]])
    src = fr.meta["frag_src"]  # of the second pass: rows of the first one, whose own frag_src leads to base
    assert fr.n > base.n + 600
    summary, layers, info = _device_parse_reasm(engine, fr, dc.OPTS)
    assert int((summary["hash5"][info["frag_offset"] > 0] != 0).sum()) == 0  # what the feature is for
    out, index, first, frags, disp, tot = defrag6_on_device(engine, fr, summary, layers, info, passthrough=True)
    assert tot["out_packets"] == base.n and tot["overflow"] == 0 and tot["left_frags"] == 0
    assert tot["reassembled"] == int((frags != 0).sum()) > 500 and tot["merged_frags"] == tot["candidates"]
    v6, ip_off, hdr, pay, _, _ = frag.locate_ipv6(base)
    assert int((frags[v6] != 0).sum()) > 200 and int((frags[~v6] != 0).sum()) > 200
    # the expected bytes: the original packets; a reassembled IPv4 one with DF cleared and its checksum recomputed, an
    # IPv6 one with the payload-length clamp where T + H byte-swapped falls below T (constructed: none of these sizes
    # does but the rule is applied to all) and its Hop-by-Hop header cut
    pk = _expected_round_trip(base, fr, frags)
    assert [out.packet(j) for j in range(base.n)] == pk
    want = from_packets(pk)
    got_s, got_l = parse_on_device(engine, out, dc.OPTS)
    want_s, want_l = oracle.oracle_parse(want, dc.OPTS)
    oracle.compare_exact(got_s, got_l, want_s, want_l)
    base_s, _ = oracle.oracle_parse(base, dc.OPTS)
    # the clamped ones (UDP of 1488 bytes behind 48 header bytes: the field says 6) are what the reference's caller
    # gets too: their parse stops short of the L4 layer, as the oracle's parse of the expected bytes just showed
    clamped = np.array([bool(frags[j]) and bool(v6[j]) and
                        int.from_bytes(pk[j][ip_off[j] + 4:ip_off[j] + 6], "big") != int(pay[j]) for j in range(base.n)])
    assert 10 < int(clamped.sum()) < 200
    # nor is a reassembled packet that had a Hop-by-Hop header the packet it was: removeAllExtensions cut that too
    # (its expected bytes, above, are without it), and its L4 layer now follows the fixed header
    cut = (hdr > 40) & (frags != 0)
    assert int(cut.sum()) > 20
    same = ~clamped & ~cut
    assert (got_s["hash5"][same] == base_s["hash5"][same]).all()
    assert (got_s["l4_layer"][same] == base_s["l4_layer"][same]).all()
    l4 = (np.arange(base.n) != 3) & same & (base_s["l4_layer"] != 0xFF)
    assert int(l4.sum()) > 1000 and (got_s["hash5"][l4] != 0).all()
    assert (got_s["hash5"][cut & ~clamped] != 0).all()
    # only the IPv4 groups with families = V4, as pcppx_defrag_device
    out4, _, _, frags4, _, tot4 = defrag6_on_device(engine, fr, summary, layers, info, families=V4)
    assert tot4["reassembled"] == int((frags[~v6] != 0).sum()) and tot4["left_frags"] > 500
