"""pcppx_frag6_device: the IPv4 and IPv6 packets of a device batch split into fragments (include/pcppx.h, frag6).

CPU: the ctypes mirrors match the header and every bad-argument combination is refused before any device work;
pcppx_frag6_reference equals a brute-force Python restatement of the contract on every case family of
tests/frag6_cases.py, byte for byte, the 0xA5 fill of everything else included; on its domain it equals
pcapplusplus_amd.frag.fragment6(), the numpy fragmenter; with families = V4 it equals pcppx_frag_reference on every
case of tests/frag_cases.py; both models reproduce the fragments recorded from the reference's own routine
(tests/golden/frag6/expected.npz); frag6 -> parse -> defrag6 through the host references gives what the model of the
reference's reassembly predicts, and the packets themselves where that can hold.
GPU: pcppx_frag6_device equals pcppx_frag6_reference byte for byte on the same cases, the gap of an IPv6 fragment at
every destination residue mod 16 among them; families = V4 is pcppx_frag_device bit for bit; two streams and a repeat
agree; a source on both sides of offset 2^32; frag6 -> parse + reasm -> defrag6, all on the device; a batch of more
blocks than one step of the base scan takes, and defrag6 on the device over its fragments.
"""
from __future__ import annotations

import ctypes as C
import functools
import re
import subprocess
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import defrag6_cases as d6
import defrag_cases as dc
import frag6_cases as f6
import frag_cases as fc
import oracle
from conftest import GOLDEN
from pcapplusplus_amd import abi, frag
from pcapplusplus_amd.pcap import PacketBatch

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
RECORDED = GOLDEN / "frag6" / "expected.npz"
CASES = f6.cases()
BY_NAME = {c.name: c for c in CASES}
V4_CASES = fc.cases()
V4, V6 = f6.V4, f6.V6
_REF: dict[str, f6.Buffers] = {}


def reference(case) -> f6.Buffers:
    """pcppx_frag6_reference's output of a case, computed once (the tests only read it)."""
    if case is not BY_NAME.get(case.name):
        return f6.run_reference(case)
    if case.name not in _REF:
        _REF[case.name] = f6.run_reference(case)
    return _REF[case.name]


# ---------------------------------------------------------------- CPU: the ABI
def test_frag6_struct_matches_header():
    cls = abi.Frag6Spec
    lines = "".join(f'  printf("{f} %zu %zu\\n", offsetof(pcppx_frag6_spec, {f}), '
                    f'sizeof(((pcppx_frag6_spec*)0)->{f}));\n' for f, _ in cls._fields_)
    consts = ["PCPPX_FRAG_FAM_V4", "PCPPX_FRAG_FAM_V6", "PCPPX_FRAG6_MAX_EXT", "PCPPX_FRAG_NOT_IP", "PCPPX_FRAG_NOT_V4",
              "PCPPX_FRAG_LEFT", "PCPPX_FRAG_BAD_DESC", "PCPPX_ABI_VERSION"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu\\n", sizeof(pcppx_frag6_spec), sizeof(pcppx_frag_spec));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(cls), C.sizeof(abi.FragSpec)]
    assert [int(x) for x in out[1].split()] == [abi.FRAG_FAM_V4, abi.FRAG_FAM_V6, abi.FRAG6_MAX_EXT, abi.FRAG_NOT_IP,
                                                abi.FRAG_NOT_V4, abi.FRAG_LEFT, abi.FRAG_BAD_DESC, abi.ABI_VERSION]
    assert (abi.FRAG_FAM_V4, abi.FRAG_FAM_V6, abi.FRAG_LEFT, abi.FRAG6_MAX_EXT, abi.ABI_VERSION) == (1, 2, 7, 16, 7)
    for line in out[2:]:
        name, off, size = line.split()
        d = getattr(cls, name)
        assert (d.offset, d.size) == (int(off), int(size)), name
    assert len(out) - 2 == len(cls._fields_)
    # pcppx_frag_spec's fields lie where they did
    for f, _ in abi.FragSpec._fields_[:5]:
        assert getattr(cls, f).offset == getattr(abi.FragSpec, f).offset, f


def test_frag6_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_frag6_device", "pcppx_frag6_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_frag6_spec(frag_size=128)
    o = abi.Fragmented(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _sizes(a, frag_size, mtu):
    a["s"].frag_size, a["s"].mtu = frag_size, mtu


def _spec_reserved(a, k):
    a["s"].reserved[k] = 1


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_offsets": lambda a: _set(a, "o", "offsets", None),
    "null_caplens": lambda a: _set(a, "o", "caplens", None),
    "null_layers": lambda a: _set(a, "r", "layers", None),
    "null_summary_and_brief": lambda a: _set(a, "r", "summary", None),
    "null_batch_offsets": lambda a: _set(a, "b", "offsets", None),
    "null_batch_caplens": lambda a: _set(a, "b", "caplens", None),
    "null_batch_data": lambda a: _set(a, "b", "data", None),
    "packed_records": lambda a: _set(a, "r", "layout", abi.LAYOUT_PACKED),
    "dense_records": lambda a: _set(a, "r", "layout", abi.LAYOUT_DENSE),
    "max_layers_0": lambda a: a.update(ml=0),
    "max_layers_17": lambda a: a.update(ml=17),
    "max_layers_255": lambda a: a.update(ml=255),
    "size_and_mtu_zero": lambda a: _sizes(a, 0, 0),
    "size_and_mtu_set": lambda a: _sizes(a, 128, 576),
    "size_not_multiple_of_8": lambda a: _sizes(a, 60, 0),
    "size_4": lambda a: _sizes(a, 4, 0),
    "size_65536": lambda a: _sizes(a, 65536, 0),
    "size_2_to_31": lambda a: _sizes(a, 1 << 31, 0),
    "mtu_67": lambda a: _sizes(a, 0, 67),
    "mtu_65536": lambda a: _sizes(a, 0, 65536),
    "copy_rest_2": lambda a: _set(a, "s", "copy_rest", 2),
    "honor_df_2": lambda a: _set(a, "s", "honor_df", 2),
    "spec_reserved_0": lambda a: _spec_reserved(a, 0),
    "spec_reserved_4": lambda a: _spec_reserved(a, 4),
    "spec_reserved2": lambda a: _set(a, "s", "reserved2", 1),
    "out_reserved": lambda a: _set(a, "o", "reserved", 1),
    "families_0": lambda a: _set(a, "s", "families", 0),
    "families_4": lambda a: _set(a, "s", "families", 4),
    "families_255": lambda a: _set(a, "s", "families", 255),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_frag6_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_frag6_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_frag6_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_frag6_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    for fam in (1, 2, 3):  # every legal families value, the bounds of both sizes and an empty batch pass
        for frag_size, mtu in ((8, 0), (65528, 0), (0, 68), (0, 65535)):
            got = f6.run_reference(replace(BY_NAME["n63"], families=fam, frag_size=frag_size, mtu=mtu))
            assert int(got.totals[abi.FRAG_OVERFLOW]) == 0
    empty = reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.FRAG_TOTALS
    f6.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    got = reference(case)
    f6.assert_same(got, f6.brute(case), case.name)
    if case.name in f6.OVERFLOWING:
        assert int(got.totals[abi.FRAG_OVERFLOW]) == 1
        f6.assert_untouched(got, case.name)  # only the totals are written
        assert int(got.totals[abi.FRAG_OUT_PACKETS]) == f6.needs(case)[0]  # and they hold the would-be values
    else:
        assert int(got.totals[abi.FRAG_OVERFLOW]) == 0


@pytest.mark.parametrize("case", V4_CASES, ids=lambda c: c.name)
def test_families_v4_equals_frag_reference(case):
    """Every column and byte; ids and id_base are ignored."""
    want = fc.run_reference(case)
    ids = np.arange(case.n, dtype=np.uint32)[::-1].copy() if case.n % 2 else None
    got = f6.run_reference(f6.widen(case, V4, ids=ids, id_base=0x1234))
    f6.assert_same(got, want, case.name)


def _disp(name):
    return [int(x) for x in reference(BY_NAME[name]).disposition[:BY_NAME[name].n]]


def _v6_rows(c):
    """(source packet, destination position of the gap) per fragment of the SPLIT IPv6 packets of a case, from the
    model."""
    out = []
    rows, _ = f6.rows_of(c)
    plans = f6.plan(c)
    pos = 0
    for i, j, pkt in rows:
        d, geo = plans[i]
        if d == abi.FRAG_SPLIT and geo[4]:
            out.append((i, pos + geo[0] + geo[1]))
        pos += len(pkt)
    return out


def test_cases_cover_the_kernel_shapes():
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kFragBlockPk\s*=\s*(\d+)", txt).group(1)) == f6.BLOCK
    assert max(c.n for c in CASES) <= 3200
    S, F, A, N, L = abi.FRAG_SPLIT, abi.FRAG_FITS, abi.FRAG_ALREADY, abi.FRAG_NOT_IP, abi.FRAG_LEFT
    # one packet split into more than 64 and more than 1024 fragments: the largest payload the capture allows, fs = 8
    c = BY_NAME["jumbo"]
    o, h, pay, fs, v6, _ = f6.plan(c)[f6.JUMBO_AT][1]
    want_c = -(-(abi.MAX_CAPLEN - o - h) // 8)
    assert v6 and fs == 8 and int(c.caplens[f6.JUMBO_AT]) == abi.MAX_CAPLEN and o + h + pay == abi.MAX_CAPLEN
    got = reference(c)
    assert int(got.counts[f6.JUMBO_AT]) == want_c == -(-pay // 8) > 1024
    assert int(got.totals[abi.FRAG_OUT_BYTES]) == want_c * (o + h + 8) + pay + 63 * (14 + 40 + 8)
    c = BY_NAME["expand_151"]
    assert int(reference(c).counts[1]) == -(-f6.plan(c)[1][1][2] // 8) == 151 > 64
    # a fragment's caplen can exceed its source's
    c = BY_NAME["pay_fs_plus_1"]
    assert max(int(x) for x in reference(c).caplens[:2]) == int(c.caplens[0]) + 7
    # per fragment size: the six payloads give 1, 1, 2, 2, 2 and 3 packets, whatever the chain and the encapsulation
    for fs in (8, 16, 128, 1480):
        for ip_off in (14, 18, 22):
            c = BY_NAME[f"size{fs}_ipoff{ip_off}"]
            assert list(reference(c).counts[:18]) == [1] * 6 + [2] * 9 + [3] * 3, (fs, ip_off)
            assert {g[0] for _, g in f6.plan(c)} == {ip_off} and {g[1] for _, g in f6.plan(c)} == {40, 48, 68}
    for mtu in (68, 576, 1500):
        c = BY_NAME[f"mtu{mtu}"]
        got = reference(c)
        seen = set()
        for i, (d, (o, h, pay, fs, v6, _)) in enumerate(f6.plan(c)):
            seen.add(d)
            if h + pay <= mtu:
                assert d == F
            elif mtu < h + 16:
                assert d == L and int(got.counts[i]) == 1
            else:
                assert d == S and fs == (mtu - h - 8) & ~7 >= 8 and int(got.counts[i]) == -(-pay // fs)
        assert {S, F} <= seen and (L in seen) == (mtu == 68)
        assert max(int(x) for x in got.caplens[:int(got.totals[0])][got.frag_no[:int(got.totals[0])] > 0]) <= 18 + mtu
    # the extension walk and the family rules, one packet each
    assert _disp("ext16") == [S] and _disp("ext17") == [L] and _disp("already") == [A, A, S]
    assert _disp("mtu_left") == [L, F, S]
    assert _disp("mpls_ahead") == [L, S]  # a layer ahead that is not Ethernet, VLAN or SLL
    assert _disp("bad_records") == [N, N, N, N, N, N, N, S, S, N]
    for fam, six4, four6 in ((3, S, S), (2, N, N), (1, S, S)):
        assert _disp(f"six_in_four_f{fam}") == [six4] and _disp(f"four_in_six_f{fam}") == [four6]
    c = BY_NAME["six_in_four_f3"]  # split at the IPv4 header: the fragments are IPv4 ones, 20 bytes behind Ethernet
    assert f6.plan(c)[0][1][:2] == (14, 20) and not f6.plan(c)[0][1][4]
    c = BY_NAME["four_in_six_f3"]  # split at the inner IPv4 header, behind the IPv6 header and its Hop-by-Hop
    assert f6.plan(c)[0][1][:2] == (14 + 48, 20) and not f6.plan(c)[0][1][4]
    # the mixed batch under the three specs
    d3, d2, d1 = _disp("mixed_v4v6"), _disp("mixed_v6"), _disp("mixed_v4")
    both = [i for i in range(300) if d3[i] == S]
    assert {d2[i] for i in both} == {S, N} and {d1[i] for i in both} == {S, N}
    assert all((d2[i] == S) != (d1[i] == S) for i in both)
    # a block that puts out nothing between two that do
    cnt = reference(BY_NAME["empty_block"]).counts[:BY_NAME["empty_block"].n].astype(np.int64)
    assert cnt[:f6.BLOCK].sum() > 0 and cnt[f6.BLOCK:2 * f6.BLOCK].sum() == 0 and cnt[2 * f6.BLOCK:].sum() > 0
    # sizing, then exact
    op, ob = f6.needs(BY_NAME["cap_exact"])
    sizing = abi.frag_totals_dict(reference(BY_NAME["maxp_zero_sizing"]).totals)
    assert (sizing["out_packets"], sizing["out_bytes"], sizing["overflow"]) == (op, ob, 1)
    # the header's closed bounds, in both modes
    seen_mtu = 0
    for c in CASES:
        if c.name == "bad_desc":
            continue
        t = abi.frag_totals_dict(reference(c).totals)
        cap = c.caplens.astype(np.int64)
        F_ = c.frag_size
        if not F_:
            hdrs = [g[1] for _, g in f6.plan(c) if g is not None and g[4]]
            H = min(max(hdrs, default=40), c.mtu - 16)
            F_ = min((c.mtu - 60) & ~7, (c.mtu - H - 8) & ~7)
            seen_mtu += 1
        assert F_ >= 8
        assert t["out_packets"] <= int(np.maximum(1, -(-cap // F_)).sum()), c.name
        assert t["out_bytes"] <= int((cap + cap * cap // (4 * F_) + 1 + 8 * -(-cap // F_)).sum()), c.name
    assert seen_mtu >= 5


def test_gap_cases_cover_every_residue():
    """The 8-byte gap of an IPv6 fragment at every destination address residue mod 16, per head length; residues 9..15
    straddle a 16-B boundary."""
    for head in f6.GAP_HEADS:
        seen = set()
        for fs in (8, 24):
            c = BY_NAME[f"gap_head{head}_fs{fs}"]
            rows = _v6_rows(c)
            assert len(rows) > 60 and {g[0] + g[1] for _, g in f6.plan(c)} == {head}
            seen |= {(c.out_misalign + at) % 16 for _, at in rows}
        assert seen == set(range(16)), (head, sorted(seen))


def _ids_of(c) -> np.ndarray:
    return np.array([c.ident(i) for i in range(c.n)], np.uint32)


def test_ids_column_and_id_base_agree_and_wrap():
    c = BY_NAME["mixed_v4v6"]
    ids = _ids_of(c)
    assert int(ids[0]) == 0xFFFFFF00 and int(ids[-1]) == 299 - 256 and c.ids is None  # wraps at 2^32
    got = reference(c)
    f6.assert_same(f6.run_reference(replace(c, ids=ids, id_base=5)), got, "ids column")  # the column wins
    out = f6.output_batch(got)
    plans = f6.plan(c)
    seen = 0
    for r in range(out.n):
        i = int(got.index[r])
        d, geo = plans[i]
        if d == abi.FRAG_SPLIT and geo[4]:
            at = geo[0] + geo[1] + 4
            assert int.from_bytes(out.packet(r)[at:at + 4], "big") == int(ids[i])
            seen += i >= 256
    assert seen > 10
    other = f6.run_reference(replace(c, id_base=1))
    assert bytes(other.data) != bytes(got.data) and list(other.caplens) == list(got.caplens)


def test_reference_equals_the_numpy_fragmenter():
    """frag.fragment6() is a second model on its domain: Ethernet, up to two VLAN tags, up to 8 extensions, a size."""
    names = ["n63", "n1025", "mixed_v6", "keep_alternating", "expand_151", "already", "trailer", "plen_small",
             "plen_large", "hbh_routing_dst", "ah_12"] + [f"gap_head{h}_fs8" for h in f6.GAP_HEADS] + \
            [f"size{fs}_ipoff{o}" for fs in (8, 128) for o in (14, 18, 22)]
    for name in names:
        c = replace(BY_NAME[name], families=V6, copy_rest=True)
        assert c.linktype == f6.ETH and c.copy_rest and c.frag_size
        got = f6.run_reference(c)
        want = frag.fragment6(c.batch(), c.frag_size, _ids_of(c), select=None if c.keep is None else c.keep != 0)
        w = int(got.totals[abi.FRAG_OUT_PACKETS])
        assert w == want.n and int(got.totals[abi.FRAG_OUT_BYTES]) == int(want.caplens.sum()), name
        assert (got.offsets[:w] == want.offsets).all() and (got.caplens[:w] == want.caplens).all(), name
        assert (got.index[:w] == want.meta["frag_src"]).all() and (got.frag_no[:w] == want.meta["frag_no"]).all(), name
        assert bytes(got.data[:int(want.caplens.sum())]) == bytes(want.data[:int(want.caplens.sum())]), name


# ---------------------------------------------------------------- CPU: recorded from the reference
def _recorded(rec, name):
    lens = rec[f"{name}.lens"]
    ends = np.cumsum(lens)
    out = rec[f"{name}.out"]
    return [bytes(out[int(e - ln):int(e)]) for e, ln in zip(ends, lens)]


def test_recorded_fragments_match_both_models():
    """Every recorded byte: pcppx_frag6_reference and frag.fragment6 on the inputs the recording was made from."""
    rec = np.load(RECORDED)
    shapes = f6.quirk_cases()
    assert len(shapes) >= 21 and {k.split(".")[0] for k in rec.files} == {c.name for c in shapes}
    for c in shapes:
        assert bytes(rec[f"{c.name}.packet"]) == c.batch().packet(0), c.name
        assert list(rec[f"{c.name}.rule"]) == [c.frag_size, c.id_base, c.linktype], c.name
        want = _recorded(rec, c.name)
        got = f6.run_reference(c)
        assert int(got.totals[abi.FRAG_SPLIT_PACKETS]) == (len(want) > 1), c.name
        out = f6.output_batch(got, c.linktype)
        assert [out.packet(j) for j in range(out.n)] == want, c.name
        model = frag.fragment6(c.batch(), c.frag_size, _ids_of(c))
        assert [model.packet(j) for j in range(model.n)] == want, c.name
    counts = {c.name: len(_recorded(rec, c.name)) for c in shapes}
    assert (counts["pay_eq_fs"], counts["pay_fs_plus_1"], counts["pay_2fs"]) == (1, 2, 2)
    # the clamp: 120 + 16 counted twice makes 136 of the 200 captured bytes payload (the field says 120 behind the
    # extensions); without extensions 120
    assert sum(len(p) - 14 - 56 - 8 for p in _recorded(rec, "plen_small")) == 136
    assert sum(len(p) - 14 - 40 - 8 for p in _recorded(rec, "plen_small_no_ext")) == 120
    assert sum(len(p) - 14 - 48 - 8 for p in _recorded(rec, "plen_large")) == 200
    assert sum(len(p) - 14 - 40 - 8 for p in _recorded(rec, "trailer")) == 150  # the 11 trailer bytes are gone
    # the layers ahead: an 802.1ad type field ahead of a VLAN layer comes out as 0x8100, behind Ethernet, VLAN and SLL
    src = {c.name: c.batch().packet(0) for c in shapes}
    for name, fields in (("qinq_88a8", (12,)), ("inner_88a8", (16,)), ("both_88a8", (12, 16)), ("one_tag_88a8", (12,)),
                         ("sll_88a8", (14,)), ("sll_two_88a8", (14, 18))):
        for p in _recorded(rec, name):
            assert all(src[name][at:at + 2] == b"\x88\xa8" and p[at:at + 2] == b"\x81\x00" for at in fields), name


# ---------------------------------------------------------------- CPU: frag6, then defrag6
ROUND_TRIP_T = (1192, 1472, 600, 64, 65, 9)  # IP payloads for which defrag6's clamp min(T, bswap16(T + 48)) is inactive


def round_trip_input() -> f6.Case:
    """No extension, no trailer, at most 64 fragments each, every T with bswap16(T + 48) >= T: the identity can hold.
    IPv4 packets of tests/frag_cases.py's round trip between them."""
    rng = np.random.default_rng(17)
    v4 = fc.clean_udp(rng, 700)
    pk = []
    for k in range(1400):
        if k % 2:
            pk.append(v4[k // 2])
        else:
            pk.append(f6.v6(rng, k, ROUND_TRIP_T[k % len(ROUND_TRIP_T)], ip_off=18 if k % 4 == 0 else 14,
                            tcp=k % 3 == 0))
    return f6.make("round_trip", pk, frag_size=128, id_base=1000)


def defrag6_case_of(b: PacketBatch) -> d6.Case:
    summary, layers = oracle.oracle_parse(b, dc.OPTS)
    info = oracle.oracle_reasm(b, summary, layers)
    return d6.Case("defrag6", b.data[:int(b.caplens.sum())], b.offsets, b.caplens, summary=summary, layers=layers,
                   info=info)


def predicted(c: f6.Case) -> list[bytes]:
    """What the reference's reassembly returns for the fragments of each packet of c (defrag6's contract): an IPv4
    packet with its header fields recomputed, an IPv6 one without its extensions and with the clamped length."""
    pk = []
    for i, (d, geo) in enumerate(f6.plan(c)):
        p = bytearray(c.batch().packet(i))
        if d == abi.FRAG_SPLIT:
            o, h, pay, fs, v6, nh_at = geo
            if v6:
                nh = p[nh_at]
                for at in f6.type_fields(c, i, o):  # the first fragment's bytes ahead of the IP header
                    p[at:at + 2] = b"\x81\x00"
                p = p[:o + h + pay]
                del p[o + 40:o + h]
                p = bytearray(d6.patched6(p, o, h + 8, pay, nh))
            else:
                p = bytearray(dc.patched(p[:o + h + pay], o, h, pay))
        pk.append(bytes(p))
    return pk


def test_clamp_is_inactive_for_the_round_trip_sizes():
    swap = lambda v: ((v & 0xFF) << 8) | (v >> 8)  # noqa: E731
    for t in ROUND_TRIP_T:
        assert min(t, swap(t + 48)) == t, t
    assert min(1488, swap(1488 + 48)) == 6  # the size the identity cannot hold for


def test_frag6_then_defrag6_reference_gives_the_prediction_on_all_shapes():
    rng = np.random.default_rng(23)
    pk = f6.mixed(rng, 400) + [f6.v6(rng, 9, 1488), f6.v6(rng, 10, 300, trailer=b"\1\2\3"),
                               f6.v6(rng, 11, 700, exts=(0, (51, 1)), ip_off=22)]
    c = f6.make("shapes", pk, frag_size=64, id_base=50)
    got = f6.run_reference(c)
    back = d6.run_reference(defrag6_case_of(f6.output_batch(got)))
    bt = abi.defrag_totals_dict(back.totals)
    already = [i for i, (d, _) in enumerate(f6.plan(c)) if d == abi.FRAG_ALREADY]
    assert bt["out_packets"] == c.n and bt["reassembled"] == int(got.totals[abi.FRAG_SPLIT_PACKETS]) > 100
    assert bt["left_frags"] == len(already) > 0  # the fragments that were in the input, never re-fragmented
    out = PacketBatch(back.data, back.offsets[:c.n], back.caplens[:c.n])
    want = predicted(c)
    for j in range(c.n):
        assert out.packet(j) == want[j], j
    assert want[c.n - 3] != c.batch().packet(c.n - 3)  # T = 1488: the clamp is active, the field says 6


def test_frag6_then_defrag6_reference_is_the_identity():
    c = round_trip_input()
    got = f6.run_reference(c)
    t = abi.frag_totals_dict(got.totals)
    v6 = np.array([bool(g and g[4]) for _, g in f6.plan(c)])
    split = got.disposition[:c.n] == abi.FRAG_SPLIT
    assert int((split & v6).sum()) > 300 and int((split & ~v6).sum()) > 200
    assert max(int(x) for x in got.counts[:c.n]) <= abi.DEFRAG_MAX_FRAGS
    back = d6.run_reference(defrag6_case_of(f6.output_batch(got)))
    bt = abi.defrag_totals_dict(back.totals)
    assert bt["left_frags"] == 0 and bt["reassembled"] == t["split_packets"] and bt["merged_frags"] == t["fragments"]
    assert bt["out_packets"] == c.n and bt["out_bytes"] == len(c.data)
    assert (back.offsets[:c.n] == c.offsets).all() and (back.caplens[:c.n] == c.caplens).all()
    assert bytes(back.data[:len(c.data)]) == bytes(c.data)


def capture_case(b: PacketBatch, name: str, **kw) -> f6.Case:
    c = fc.over(name, b.data[:int(b.caplens.sum())], b.offsets, b.caplens, b.linktype)
    return replace(f6.widen(c, V4 | V6), **kw)


def test_fragmenting_the_fragments_changes_nothing_reference():
    c = BY_NAME["n1025"]
    once = reference(c)
    b = f6.output_batch(once)
    again = f6.run_reference(capture_case(b, "again", frag_size=c.frag_size))
    w = int(once.totals[abi.FRAG_OUT_PACKETS])
    assert int(again.totals[abi.FRAG_SPLIT_PACKETS]) == 0 and int(again.totals[abi.FRAG_OUT_PACKETS]) == w
    frags = np.repeat(once.disposition[:c.n] == abi.FRAG_SPLIT, once.counts[:c.n])
    assert (again.disposition[:w][frags] == abi.FRAG_ALREADY).all() and frags.sum() > 500
    assert bytes(again.data[:int(again.totals[1])]) == bytes(once.data[:int(once.totals[1])])


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_frag6_equals_reference(engine, case):
    want = reference(case)
    got = f6.run_device(engine, case)
    f6.assert_same(got, want, case.name)
    if case.name in f6.OVERFLOWING:
        f6.assert_untouched(got, case.name)


@pytest.mark.gpu
def test_gpu_recorded_fragments_on_the_device(engine):
    rec = np.load(RECORDED)
    for c in f6.quirk_cases():
        out = f6.output_batch(f6.run_device(engine, c), c.linktype)
        assert [out.packet(j) for j in range(out.n)] == _recorded(rec, c.name), c.name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1025", "jumbo_8190", "mtu576", "bad_desc_rest1", "keep_alternating_only"])
def test_gpu_families_v4_is_bit_identical_to_frag_device(engine, name):
    case = next(c for c in V4_CASES if c.name == name)
    want = fc.run_device(engine, case)
    got = f6.run_device(engine, f6.widen(case, V4, id_base=77))
    f6.assert_same(got, want, name)
    f6.assert_same(got, fc.run_reference(case), name)
    c6 = BY_NAME["mixed_v4"]  # and on a batch that holds IPv6 packets
    as_v4 = fc.Case(**{f: getattr(c6, f) for f in fc.Case.__dataclass_fields__})
    f6.assert_same(f6.run_device(engine, c6), fc.run_device(engine, as_v4), "mixed_v4")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n2049", "jumbo", "empty_block", "cap_short1", "mtu576", "gap_head70_fs8"])
def test_gpu_frag6_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = reference(case)
    runs = [f6.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        f6.assert_same(r.result(), want, f"{name} run {k}")


@pytest.mark.gpu
def test_gpu_sizing_call_then_exact_size_call(engine):
    """frag6_on_device makes the index-only sizing call (max_packets = 0) and then the call with exactly that room."""
    from pcapplusplus_amd.engine import frag6_on_device

    for name in ("mixed_v4v6", "mixed_mtu_brief", "mixed_v6"):
        c = BY_NAME[name]
        want = reference(c)
        w, wb = int(want.totals[abi.FRAG_OUT_PACKETS]), int(want.totals[abi.FRAG_OUT_BYTES])
        out, index, frag_no, disp, tot = frag6_on_device(engine, c.batch(), c.summary, c.layers, c.frag_size, c.mtu,
                                                         c.families, None, c.id_base, copy_rest=c.copy_rest)
        assert (tot["out_packets"], tot["out_bytes"], tot["overflow"]) == (w, wb, 0), name
        assert len(out.data) == wb and bytes(out.data) == bytes(want.data[:wb]), name
        assert (out.offsets == want.offsets[:w]).all() and (out.caplens == want.caplens[:w]).all(), name
        assert (index == want.index[:w]).all() and (frag_no == want.frag_no[:w]).all(), name
        assert (disp == want.disposition[:c.n]).all(), name
    c = BY_NAME["n63"]  # an ids column through the wrapper
    out, *_ = frag6_on_device(engine, c.batch(), c.summary, c.layers, c.frag_size, ids=c.ids)
    want = reference(c)
    assert bytes(out.data) == bytes(want.data[:int(want.totals[abi.FRAG_OUT_BYTES])])


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 9])
def test_gpu_frag6_source_on_both_sides_of_4gib(engine, mis):
    """test_gpu_frag_source_on_both_sides_of_4gib for a batch of both families: a split IPv6 packet lies across each
    line."""
    import torch

    import wide_cases as wc

    case = replace(BY_NAME["n1025"], src_misalign=0, out_misalign=3)
    plans = f6.plan(case)
    raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device="cuda:0")
    lay = wc.layout(raw.data_ptr(), mis)
    data = raw[lay.pad: lay.pad + lay.data_len]
    n, half = case.n, case.n // 2
    lens = case.caplens.astype(np.int64)
    offs = np.zeros(n, np.int64)
    for lo, hi, line in ((0, half, lay.lines[0]), (half, n, lay.lines[1])):
        run = np.cumsum(lens[lo:hi]) - lens[lo:hi]
        mid = (lo + hi) // 2 - lo
        while not (plans[lo + mid][0] == abi.FRAG_SPLIT and plans[lo + mid][1][4]):  # a split IPv6 packet
            mid += 1
        start = line - int(run[mid]) - int(lens[lo + mid]) // 2
        offs[lo:hi] = start + run
        k = lo + mid
        assert offs[k] < line < offs[k] + lens[k]
        src0 = int(case.offsets[lo])
        chunk = case.data[src0:src0 + int(lens[lo:hi].sum())]
        data[start:start + len(chunk)] = torch.from_numpy(chunk).to("cuda:0")
    order = np.random.default_rng(5).permutation(n)  # descriptors of both sides interleaved
    wide = fc.permuted(replace(case, offsets=offs.astype(np.uint64), ids=case.ids[order]), order)
    compact = fc.permuted(replace(case, ids=case.ids[order]), order)
    source = (data, torch.from_numpy(wide.offsets.view(np.int64)).to("cuda:0"),
              torch.from_numpy(wide.caplens.view(np.int32)).to("cuda:0"), lay.data_len)
    want = f6.run_reference(compact)
    assert int(want.totals[abi.FRAG_SPLIT_PACKETS]) > 100
    assert {bool(o < wc.LINE) for o in wide.offsets} == {True, False}
    got = f6.run_device(engine, compact, source=source)
    f6.assert_same(got, want, f"wide mis{mis}")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_frag6_defrag6_round_trip_on_the_device(engine):
    """frag6 (copy_rest = 1) -> pcppx_parse_batch_device_reasm -> defrag6 (passthrough = 1), nothing leaving the device
    in between: the batch of both families comes back byte for byte and descriptor for descriptor."""
    import torch

    c = round_trip_input()
    st = torch.cuda.current_stream().cuda_stream
    run = f6.DeviceRun(c)
    run.launch(engine, st)
    fr = run.result()
    t = abi.frag_totals_dict(fr.totals)
    assert t["overflow"] == 0 and t["split_packets"] > 500
    w, wb = t["out_packets"], t["out_bytes"]
    f_data, f_off, f_cap = run.d_data[:wb + 1], run.d_off[:w], run.d_cap[:w]  # the fragmented batch, in HBM
    summary = torch.zeros(w * 32, dtype=torch.uint8, device="cuda:0")
    layers = torch.zeros(w * dc.OPTS.max_layers * 8, dtype=torch.uint8, device="cuda:0")
    info = torch.zeros(w * 16, dtype=torch.uint8, device="cuda:0")
    engine.parse_reasm_device(f_data, f_off, f_cap, w, fc.ETH, dc.OPTS, summary, layers, info, st)
    back = dc.alloc(dc.Case("back", c.data, c.offsets, c.caplens))
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to("cuda:0")  # noqa: E731
    o_data, o_off, o_cap = up(back.data, np.uint8), up(back.offsets, np.int64), up(back.caplens, np.int32)
    o_disp = torch.zeros(w, dtype=torch.uint8, device="cuda:0")
    o_tot = up(back.totals, np.int64)
    engine.defrag6_device(f_data, f_off, f_cap, w, fc.ETH, layers, dc.ML, info, abi.make_defrag6_spec(True, 0), o_off,
                          o_cap, o_tot, c.n, o_data, len(c.data), disposition=o_disp, stream=st, data_len=wb,
                          summary=summary)
    torch.cuda.synchronize()
    bt = abi.defrag_totals_dict(o_tot.cpu().numpy().view(np.uint64))
    assert bt["overflow"] == 0 and bt["left_frags"] == 0 and bt["reassembled"] == t["split_packets"]
    assert bt["out_packets"] == c.n and bt["out_bytes"] == len(c.data)
    got_off, got_cap = o_off.cpu().numpy().view(np.uint64), o_cap.cpu().numpy().view(np.uint32)
    got_data = o_data.cpu().numpy()
    assert (got_off[:c.n] == c.offsets).all() and (got_cap[:c.n] == c.caplens).all()
    assert bytes(got_data[:len(c.data)]) == bytes(c.data) and (got_data[len(c.data):] == fc.FILL).all()


@pytest.mark.gpu
def test_gpu_fragmenting_the_fragments_changes_nothing(engine):
    from pcapplusplus_amd.engine import frag6_on_device, parse_on_device

    c = BY_NAME["n1025"]
    once = f6.run_device(engine, c)
    b = f6.output_batch(once)
    summary, layers = parse_on_device(engine, b, dc.OPTS)
    out, index, frag_no, disp, tot = frag6_on_device(engine, b, summary, layers, frag_size=c.frag_size)
    frags = np.repeat(once.disposition[:c.n] == abi.FRAG_SPLIT, once.counts[:c.n])
    assert tot["split_packets"] == 0 and tot["overflow"] == 0 and out.n == b.n and frags.sum() > 500
    assert (disp[frags] == abi.FRAG_ALREADY).all() and (index == np.arange(b.n)).all() and not frag_no.any()
    assert bytes(out.data) == bytes(b.data[:int(b.caplens.sum())])


# ---------------------------------------------------------------- the base scan's second step
N_WIDE, STEP = 66 * fc.BLOCK + 7, 64  # blocks a step of the base kernel takes
WIDE_TOTALS = {"out_packets": 127180, "out_bytes": 19350162, "split_packets": 11511, "fragments": 71100,
               "copied": 56080, "under_size": 52372}  # frozen; none is zero: every carried sum is used


@functools.lru_cache(maxsize=None)
def wide():
    """(the 67-block case, what the reference leaves): built once, shared by the CPU and the GPU test."""
    case = f6.make("wide", f6.mixed(np.random.default_rng(32), N_WIDE), frag_size=128, id_base=7)
    return case, f6.run_reference(case)


def test_reference_past_64_blocks():
    case, want = wide()
    assert case.n == N_WIDE and (N_WIDE + fc.BLOCK - 1) // fc.BLOCK == STEP + 3
    f6.assert_same(want, f6.brute(case), "wide")
    totals = abi.frag_totals_dict(want.totals)
    assert totals["overflow"] == 0 and totals["bad_desc"] == 0
    cnt = want.counts[:N_WIDE].astype(np.int64)
    split = want.disposition[:N_WIDE] == abi.FRAG_SPLIT
    for blk in (STEP, STEP + 1):  # the blocks behind the step line put packets out, fragments among them
        rows = slice(blk * fc.BLOCK, (blk + 1) * fc.BLOCK)
        assert int(cnt[rows].sum()) > fc.BLOCK and int(split[rows].sum()) >= 1, blk
    assert all(v != 0 for v in WIDE_TOTALS.values()) and {k: totals[k] for k in WIDE_TOTALS} == WIDE_TOTALS


@pytest.mark.gpu
def test_gpu_frag6_past_64_blocks(engine):
    """The device equals the reference; and defrag6 on the device over the fragmented batch, whose groups then lie on
    both sides of the step line of defrag's own scan, equals defrag6's reference."""
    case, want = wide()
    got = f6.run_device(engine, case)
    f6.assert_same(got, want, "wide")
    back = defrag6_case_of(f6.output_batch(got))
    ref = d6.run_reference(back)
    t = abi.defrag_totals_dict(ref.totals)
    assert back.n == WIDE_TOTALS["out_packets"] > (STEP + 1) * dc.BLOCK and t["overflow"] == 0
    assert t["reassembled"] > 8000 and t["out_packets"] > (STEP + 1) * dc.BLOCK
    d6.assert_same(d6.run_device(engine, back), ref, "wide, defragmented")
