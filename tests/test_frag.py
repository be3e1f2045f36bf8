"""pcppx_frag_device: the IPv4 packets of a device batch split into fragments (include/pcppx.h, frag).

CPU: the ctypes mirrors match the header and every bad-argument combination is refused before any device work;
pcppx_frag_reference (the contract in plain C++ over host pointers) equals a brute-force Python restatement of the
contract on every case family of tests/frag_cases.py, byte for byte, the 0xA5 fill of everything else included (all of it
but the totals on overflow); on Ethernet / VLAN batches it also equals pcapplusplus_amd.frag.fragment(), the numpy
fragmenter; it reproduces the reference's own IPFragUtil vectors (tests/golden/ingest/files, tests/golden/frag); and
frag -> parse -> defrag through the three host references gives the batch back.
GPU: pcppx_frag_device equals pcppx_frag_reference byte for byte on the same cases; two calls on two streams agree and
a repeat is bit-identical; source packets on both sides of offset 2^32; the reference's vectors on the device; frag ->
parse + reasm -> defrag, all on the device, is the identity; fragmenting the fragments again changes nothing; a batch of
more blocks than one step of the base scan takes, and defrag on the device over its fragments.
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

import defrag_cases as dc
import frag_cases as fc
import oracle
from conftest import GOLDEN
from pcapplusplus_amd import abi, frag
from pcapplusplus_amd.pcap import PacketBatch, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
FILES = GOLDEN / "ingest" / "files"
CASES = fc.cases()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- CPU: the ABI
def test_frag_structs_match_header():
    fields = {"pcppx_frag_spec": abi.FragSpec, "pcppx_fragmented": abi.Fragmented}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = ["PCPPX_FRAG_UNSELECTED", "PCPPX_FRAG_NOT_V4", "PCPPX_FRAG_ALREADY", "PCPPX_FRAG_FITS", "PCPPX_FRAG_DF",
              "PCPPX_FRAG_SPLIT", "PCPPX_FRAG_BAD_DESC", "PCPPX_FRAG_OUT_PACKETS", "PCPPX_FRAG_OUT_BYTES",
              "PCPPX_FRAG_SPLIT_PACKETS", "PCPPX_FRAG_FRAGMENTS", "PCPPX_FRAG_COPIED", "PCPPX_FRAG_UNDER_SIZE",
              "PCPPX_FRAG_BAD_DESC_N", "PCPPX_FRAG_OVERFLOW", "PCPPX_FRAG_TOTALS", "PCPPX_ABI_VERSION"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu\\n", sizeof(pcppx_frag_spec), sizeof(pcppx_fragmented));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.FragSpec), C.sizeof(abi.Fragmented)]
    assert [int(x) for x in out[1].split()] == [
        abi.FRAG_UNSELECTED, abi.FRAG_NOT_V4, abi.FRAG_ALREADY, abi.FRAG_FITS, abi.FRAG_DF, abi.FRAG_SPLIT,
        abi.FRAG_BAD_DESC, abi.FRAG_OUT_PACKETS, abi.FRAG_OUT_BYTES, abi.FRAG_SPLIT_PACKETS, abi.FRAG_FRAGMENTS,
        abi.FRAG_COPIED, abi.FRAG_UNDER_SIZE, abi.FRAG_BAD_DESC_N, abi.FRAG_OVERFLOW, abi.FRAG_TOTALS, abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        seen += 1
    assert seen == len(abi.FragSpec._fields_) + len(abi.Fragmented._fields_)
    assert abi.ABI_VERSION == 7 and len(abi.FRAG_FIELDS) == abi.FRAG_TOTALS


def test_frag_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_frag_device", "pcppx_frag_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_frag_spec(frag_size=128)
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
    "spec_reserved_5": lambda a: _spec_reserved(a, 5),
    "out_reserved": lambda a: _set(a, "o", "reserved", 1),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_frag_device's, pcppx_frag_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_frag_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_frag_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_frag_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_frag_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # the bounds of both sizes, a brief instead of the summary, absent optional columns and an empty batch pass
    for frag_size, mtu in ((8, 0), (65528, 0), (0, 68), (0, 65535)):
        got = fc.run_reference(replace(BY_NAME["n63"], frag_size=frag_size, mtu=mtu))
        assert int(got.totals[abi.FRAG_OVERFLOW]) == 0
    for name in ("keep_alternating_only", "no_columns", "n0"):
        assert int(fc.run_reference(BY_NAME[name]).totals[abi.FRAG_OVERFLOW]) == 0
    empty = fc.run_reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.FRAG_TOTALS
    fc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    got = fc.run_reference(case)
    fc.assert_same(got, fc.brute(case), case.name)
    if case.name in fc.OVERFLOWING:
        assert int(got.totals[abi.FRAG_OVERFLOW]) == 1
        fc.assert_untouched(got, case.name)
    else:
        assert int(got.totals[abi.FRAG_OVERFLOW]) == 0


def _disp(name):
    c = BY_NAME[name]
    return [d for d, _ in fc.plan(c)]


def test_cases_cover_the_kernel_shapes():
    """The block size the cases are built around is the kernels', and the families reach the paths they name."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kFragBlockPk\s*=\s*(\d+)", txt).group(1)) == fc.BLOCK
    assert max(c.n for c in CASES) <= 3200
    t = abi.frag_totals_dict(fc.brute(BY_NAME["expand_185"]).totals)
    assert (t["split_packets"], t["fragments"], t["out_packets"]) == (1, 185, 187)
    for name, frags in (("jumbo_8190", 8190), ("jumbo_only_fragments", 1365)):
        got = fc.brute(BY_NAME[name])
        t = abi.frag_totals_dict(got.totals)
        assert (t["split_packets"], t["fragments"]) == (1, frags) and frags > 64
        assert int(got.counts[fc.JUMBO_AT]) == frags and BY_NAME[name].n == 64
    assert abi.frag_totals_dict(fc.brute(BY_NAME["jumbo_8190"]).totals)["out_packets"] == 8190 + 63 > fc.BLOCK
    # per fragment size: the six payloads give 1, 1, 2, 2, 2 and 3 packets, whatever the header and the encapsulation
    for fs in (8, 16, 128, 1480):
        for ip_off in (0, 14, 16, 18, 22):
            got = fc.brute(BY_NAME[f"size{fs}_ipoff{ip_off}"])
            assert list(got.counts[:18]) == [1] * 6 + [2] * 9 + [3] * 3, (fs, ip_off)
            c = BY_NAME[f"size{fs}_ipoff{ip_off}"]
            assert {g[0] for _, g in fc.plan(c)} == {ip_off} and {g[1] for _, g in fc.plan(c)} == {20, 24, 60}
    t = abi.frag_totals_dict(fc.brute(BY_NAME["size65528"]).totals)
    assert (t["under_size"], t["split_packets"]) == (3, 0)
    for mtu in (68, 576, 1500):
        c = BY_NAME[f"mtu{mtu}"]
        got = fc.brute(c)
        for i, (d, (o, h, pay, fs)) in enumerate(fc.plan(c)):
            assert fs == (mtu - h) & ~7 and (d == abi.FRAG_SPLIT) == (h + pay > mtu)
            assert int(got.counts[i]) == (-(-pay // fs) if h + pay > mtu else 1)
        assert max(int(x) for x in got.caplens[:int(got.totals[0])]) <= 22 + mtu  # no fragment exceeds the MTU
    # a block that puts out nothing between two that do
    got = fc.brute(BY_NAME["empty_block"])
    cnt = got.counts[:BY_NAME["empty_block"].n].astype(np.int64)
    assert cnt[:fc.BLOCK].sum() > 0 and cnt[fc.BLOCK:2 * fc.BLOCK].sum() == 0 and cnt[2 * fc.BLOCK:].sum() > 0
    # every disposition, DF with and without honor_df, the three kinds of fragments, IPv6 with and without a fragment header
    d0, d1 = _disp("dispositions_df0"), _disp("dispositions_df1")
    S, F, D, A, N = abi.FRAG_SPLIT, abi.FRAG_FITS, abi.FRAG_DF, abi.FRAG_ALREADY, abi.FRAG_NOT_V4
    assert d0 == [S, S, F, A, A, A, A, N, N, N] and d1 == [D, S, F, A, A, A, A, N, N, N]
    assert abi.FRAG_UNSELECTED in _disp("keep_alternating") and set(_disp("keep_none")) == {abi.FRAG_UNSELECTED}
    assert _disp("bad_records") == [N, N, N, N, N, N, N, S, A, S, S, S]  # 8: read where its record points
    for name in ("bad_desc_rest0", "bad_desc_rest1"):
        t = abi.frag_totals_dict(fc.brute(BY_NAME[name]).totals)
        assert t["bad_desc"] > 20 and t["split_packets"] > 50
    assert int(BY_NAME["bad_desc_rest0"].offsets.max()) > 1 << 63  # the 64-bit wrap
    assert _disp("overlapping").count(S) >= 16 and _disp("reversed").count(S) == 16
    t = abi.frag_totals_dict(fc.brute(BY_NAME["trailer"]).totals)
    # 300 and 129 bytes of payload are split in 3 and 2: three more 34-byte heads, their trailers (8 and 3 bytes) gone
    assert t["out_bytes"] == int(BY_NAME["trailer"].caplens.sum()) + 3 * 34 - 8 - 3 and t["split_packets"] == 2
    t = abi.frag_totals_dict(fc.brute(BY_NAME["cut_capture"]).totals)
    assert t["split_packets"] == 2 and t["under_size"] == 3  # 700 and 299 captured bytes; 1, 128 and 10
    op, ob = fc.needs(BY_NAME["cap_exact"])  # whatever its capacities
    exact = abi.frag_totals_dict(fc.brute(BY_NAME["cap_exact"]).totals)
    assert (exact["out_packets"], exact["out_bytes"], exact["overflow"]) == (op, ob, 0)
    sizing = abi.frag_totals_dict(fc.run_reference(BY_NAME["maxp_zero_sizing"]).totals)
    assert (sizing["out_packets"], sizing["out_bytes"], sizing["overflow"]) == (op, ob, 1)  # how a caller sizes
    # the header's closed bounds hold on every case
    for c in CASES:
        t = abi.frag_totals_dict(fc.brute(c).totals)
        F_ = c.frag_size or (c.mtu - 60) & ~7
        ok = (c.offsets <= np.uint64(c.dlen())) & (c.offsets + c.caplens <= np.uint64(c.dlen())) & \
            (c.offsets + c.caplens >= c.offsets)
        cap = c.caplens[ok].astype(np.int64)
        assert t["out_packets"] <= int(np.maximum(1, -(-cap // F_)).sum()), c.name
        assert t["out_bytes"] <= int((cap + cap * cap // (4 * F_) + 1).sum()), c.name


def test_reference_equals_the_numpy_fragmenter():
    """frag.fragment() is a second model on what it handles: Ethernet, up to two VLAN tags, a size, a mask."""
    for name in ("n1025", "n2049", "keep_all", "keep_alternating", "trailer", "cut_capture", "expand_185",
                 "dispositions_df0", "size128_ipoff22", "size8_ipoff14"):
        c = BY_NAME[name]
        assert c.linktype == fc.ETH and c.copy_rest and not c.honor_df
        got = fc.run_reference(c)
        want = frag.fragment(c.batch(), c.frag_size, select=None if c.keep is None else c.keep != 0)
        w = int(got.totals[abi.FRAG_OUT_PACKETS])
        assert w == want.n and int(got.totals[abi.FRAG_OUT_BYTES]) == int(want.caplens.sum()), name
        assert (got.offsets[:w] == want.offsets).all() and (got.caplens[:w] == want.caplens).all(), name
        assert (got.index[:w] == want.meta["frag_src"]).all() and (got.frag_no[:w] == want.meta["frag_no"]).all(), name
        assert (got.counts[:c.n] == np.bincount(want.meta["frag_src"], minlength=c.n)).all(), name
        assert bytes(got.data[:int(want.caplens.sum())]) == bytes(want.data[:int(want.caplens.sum())]), name


# ---------------------------------------------------------------- CPU: the reference's own vectors
def capture_case(b: PacketBatch, name: str, **kw) -> fc.Case:
    c = fc.over(name, b.data[:int(b.caplens.sum())], b.offsets, b.caplens, b.linktype, **kw)
    c.meta["batch"] = b
    return c


def _be16(b: PacketBatch, i: int, at: int) -> int:
    return int.from_bytes(b.packet(i)[at:at + 2], "big")


def vector_cases() -> list[tuple[fc.Case, PacketBatch]]:
    """(case, the records IPFragUtil wrote) of the reference's three runs (Tests/ExamplesTest/tests/test_ipfragutil.py)."""
    out = []
    b = read_pcap(FILES / "Tests__ExamplesTest__pcap_examples__http_req.pcap")
    out.append((capture_case(b, "http_req", frag_size=128, copy_rest=False),
                read_pcap(FILES / "Tests__ExamplesTest__expected_output__http_req_frag.pcap")))
    b = read_pcap(GOLDEN / "frag" / "http_packets_subset.pcap")  # tools/make_golden_frag.py
    assert all(b.packet(i)[12:14] == b"\x08\x00" and b.packet(i)[14] == 0x45 for i in range(b.n))
    ids = np.array([_be16(b, i, 18) in (22574, 22582) for i in range(b.n)])  # -d 22574,22582
    port = np.array([b.packet(i)[23] == 6 and _be16(b, i, 34) == 8881 for i in range(b.n)])  # -f "tcp src port 8881"
    assert int(ids.sum()) == 2 and int(port.sum()) == 5
    out.append((capture_case(b, "ip_ids", frag_size=256, copy_rest=False, keep=ids.astype(np.uint8)),
                read_pcap(FILES / "Tests__ExamplesTest__expected_output__ipfragutil_ip_ids.pcap")))
    out.append((capture_case(b, "bpf_filter", frag_size=256, copy_rest=False, keep=port.astype(np.uint8)),
                read_pcap(FILES / "Tests__ExamplesTest__expected_output__ipfragutil_bpf_filter.pcap")))
    return out


def assert_is_vector(c: fc.Case, got: fc.Buffers, want: PacketBatch) -> None:
    """The output's records are the file's: bytes, caplens, frame lengths and timestamps."""
    src = c.meta["batch"]
    w = int(got.totals[abi.FRAG_OUT_PACKETS])
    assert w == want.n and int(got.totals[abi.FRAG_OVERFLOW]) == 0, c.name
    out = fc.output_batch(got)
    assert [out.packet(j) for j in range(w)] == [want.packet(j) for j in range(w)], c.name
    assert (got.caplens[:w] == want.caplens).all() and (got.caplens[:w] == want.frame_lens).all(), c.name
    assert (src.timestamps_ns[got.index[:w]] == want.timestamps_ns).all(), c.name


def test_reference_on_the_vectors():
    for c, want in vector_cases():
        d = [x for x, _ in fc.plan(replace(c, keep=None))]
        assert abi.FRAG_ALREADY not in d and abi.FRAG_NOT_V4 not in d  # the two departures do not touch the vectors
        got = fc.run_reference(c)
        assert_is_vector(c, got, want)
        fc.assert_same(got, fc.brute(c), c.name)
    sub = vector_cases()[1][0]
    d = [x for x, _ in fc.plan(replace(sub, keep=None))]
    assert d.count(abi.FRAG_SPLIT) >= 7 and d.count(abi.FRAG_FITS) >= 5  # under-size neighbours are there too
    assert abi.FRAG_UNSELECTED in [x for x, _ in fc.plan(sub)]


# ---------------------------------------------------------------- CPU: frag, then defrag
def round_trip_input() -> fc.Case:
    return fc.make("round_trip", fc.clean_udp(np.random.default_rng(11), 1500), frag_size=128)


def defrag_case_of(b: PacketBatch) -> dc.Case:
    summary, layers = oracle.oracle_parse(b, dc.OPTS)
    info = oracle.oracle_reasm(b, summary, layers)
    return dc.Case("defrag", b.data[:int(b.caplens.sum())], b.offsets, b.caplens, summary=summary, layers=layers,
                   info=info)


def test_frag_then_defrag_reference_is_the_identity():
    """What the GPU round trip relies on: on its input the reference model alone leaves no group LEFT."""
    c = round_trip_input()
    got = fc.run_reference(c)
    t = abi.frag_totals_dict(got.totals)
    assert t["split_packets"] > 500 and max(int(x) for x in got.counts[:c.n]) <= abi.DEFRAG_MAX_FRAGS
    back = dc.run_reference(defrag_case_of(fc.output_batch(got)))
    bt = abi.defrag_totals_dict(back.totals)
    assert bt["left_frags"] == 0 and bt["reassembled"] == t["split_packets"] and bt["merged_frags"] == t["fragments"]
    assert bt["out_packets"] == c.n and bt["out_bytes"] == len(c.data)
    assert (back.offsets[:c.n] == c.offsets).all() and (back.caplens[:c.n] == c.caplens).all()
    assert bytes(back.data[:len(c.data)]) == bytes(c.data)


def test_fragmenting_the_fragments_changes_nothing_reference():
    c = BY_NAME["n1025"]
    once = fc.run_reference(c)
    b = fc.output_batch(once)
    again = fc.run_reference(capture_case(b, "again", frag_size=c.frag_size))
    w = int(once.totals[abi.FRAG_OUT_PACKETS])
    assert int(again.totals[abi.FRAG_SPLIT_PACKETS]) == 0 and int(again.totals[abi.FRAG_OUT_PACKETS]) == w
    frags = np.repeat(once.disposition[:c.n] == abi.FRAG_SPLIT, once.counts[:c.n])
    assert (again.disposition[:w][frags] == abi.FRAG_ALREADY).all() and frags.sum() > 500
    assert bytes(again.data[:int(again.totals[1])]) == bytes(once.data[:int(once.totals[1])])


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_frag_equals_reference(engine, case):
    want = fc.run_reference(case)
    got = fc.run_device(engine, case)
    fc.assert_same(got, want, case.name)
    if case.name in fc.OVERFLOWING:
        fc.assert_untouched(got, case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n2049", "jumbo_8190", "empty_block", "cap_short1", "mtu576"])
def test_gpu_frag_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = fc.run_reference(case)
    runs = [fc.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        fc.assert_same(r.result(), want, f"{name} run {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 9])
def test_gpu_frag_source_on_both_sides_of_4gib(engine, mis):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32
    (the layout of test_defrag.py's case): one packet lies across each line."""
    import torch

    import wide_cases as wc

    case = replace(BY_NAME["n1025"], src_misalign=0, out_misalign=3)
    raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device="cuda:0")
    lay = wc.layout(raw.data_ptr(), mis)
    data = raw[lay.pad: lay.pad + lay.data_len]
    n, half = case.n, case.n // 2
    lens = case.caplens.astype(np.int64)
    offs = np.zeros(n, np.int64)
    for lo, hi, line in ((0, half, lay.lines[0]), (half, n, lay.lines[1])):
        run = np.cumsum(lens[lo:hi]) - lens[lo:hi]
        mid = (lo + hi) // 2 - lo
        while case.caplens[lo + mid] < 600:  # a packet that is split lies across the line
            mid += 1
        start = line - int(run[mid]) - int(lens[lo + mid]) // 2
        offs[lo:hi] = start + run
        k = lo + mid
        assert offs[k] < line < offs[k] + lens[k]
        src0 = int(case.offsets[lo])
        chunk = case.data[src0:src0 + int(lens[lo:hi].sum())]
        data[start:start + len(chunk)] = torch.from_numpy(chunk).to("cuda:0")
    order = np.random.default_rng(5).permutation(n)  # descriptors of both sides interleaved
    wide = fc.permuted(replace(case, offsets=offs.astype(np.uint64)), order)
    compact = fc.permuted(case, order)
    source = (data, torch.from_numpy(wide.offsets.view(np.int64)).to("cuda:0"),
              torch.from_numpy(wide.caplens.view(np.int32)).to("cuda:0"), lay.data_len)
    want = fc.run_reference(compact)
    assert int(want.totals[abi.FRAG_SPLIT_PACKETS]) > 100
    assert {bool(o < wc.LINE) for o in wide.offsets} == {True, False}
    got = fc.run_device(engine, compact, source=source)
    fc.assert_same(got, want, f"wide mis{mis}")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_gpu_frag_on_the_reference_vectors(engine):
    from pcapplusplus_amd.engine import frag_on_device

    for c, want in vector_cases():
        got = fc.run_device(engine, c)
        fc.assert_same(got, fc.run_reference(c), c.name)
        assert_is_vector(c, got, want)
    c, want = vector_cases()[0]
    b = c.meta["batch"]
    out, index, frag_no, disp, tot = frag_on_device(engine, b, c.summary, c.layers, frag_size=128, copy_rest=False)
    assert out.n == want.n and [out.packet(j) for j in range(out.n)] == [want.packet(j) for j in range(want.n)]
    assert (out.timestamps_ns == want.timestamps_ns).all() and (out.frame_lens == want.frame_lens).all()
    assert list(frag_no) == list(range(want.n)) and set(index) == {0} and list(disp) == [abi.FRAG_SPLIT]


def _device_parse_reasm(engine, data, offsets, caplens, n: int, opts):
    import torch

    summary = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    layers = torch.zeros(n * opts.max_layers * 8, dtype=torch.uint8, device="cuda:0")
    info = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    engine.parse_reasm_device(data, offsets, caplens, n, fc.ETH, opts, summary, layers, info,
                              torch.cuda.current_stream().cuda_stream)
    return summary, layers, info


@pytest.mark.gpu
def test_gpu_frag_defrag_round_trip_on_the_device(engine):
    """frag (copy_rest = 1) -> pcppx_parse_batch_device_reasm -> defrag (passthrough = 1), nothing leaving the device
    in between: the batch comes back byte for byte and descriptor for descriptor, and parses to the same records."""
    import torch

    from pcapplusplus_amd.engine import parse_on_device

    c = round_trip_input()
    st = torch.cuda.current_stream().cuda_stream
    run = fc.DeviceRun(c)
    run.launch(engine, st)
    fr = run.result()
    t = abi.frag_totals_dict(fr.totals)
    assert t["overflow"] == 0 and t["split_packets"] > 500
    w, wb = t["out_packets"], t["out_bytes"]
    f_data, f_off, f_cap = run.d_data[:wb + 1], run.d_off[:w], run.d_cap[:w]  # the fragmented batch, in HBM
    summary, layers, info = _device_parse_reasm(engine, f_data, f_off, f_cap, w, dc.OPTS)
    back = dc.alloc(dc.Case("back", c.data, c.offsets, c.caplens))
    up = lambda a, dt: torch.from_numpy(a.view(dt)).to("cuda:0")  # noqa: E731
    o_data, o_off, o_cap = up(back.data, np.uint8), up(back.offsets, np.int64), up(back.caplens, np.int32)
    o_disp = torch.zeros(w, dtype=torch.uint8, device="cuda:0")
    o_tot = up(back.totals, np.int64)
    engine.defrag_device(f_data, f_off, f_cap, w, fc.ETH, layers, dc.ML, info, abi.make_defrag_spec(True, 0), o_off,
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
    out = PacketBatch(np.concatenate([got_data[:len(c.data)], np.zeros(1, np.uint8)]), got_off[:c.n].copy(),
                      got_cap[:c.n].copy())
    got_s, got_l = parse_on_device(engine, out, dc.OPTS)
    oracle.compare_exact(got_s, got_l, c.summary, c.layers)
    assert (got_s["hash5"] == c.summary["hash5"]).all() and int((got_s["hash5"] != 0).sum()) > c.n * 9 // 10


@pytest.mark.gpu
def test_gpu_fragmenting_the_fragments_changes_nothing(engine):
    from pcapplusplus_amd.engine import frag_on_device, parse_on_device

    c = BY_NAME["n1025"]
    once = fc.run_device(engine, c)
    b = fc.output_batch(once)
    summary, layers = parse_on_device(engine, b, dc.OPTS)
    out, index, frag_no, disp, tot = frag_on_device(engine, b, summary, layers, frag_size=c.frag_size)
    frags = np.repeat(once.disposition[:c.n] == abi.FRAG_SPLIT, once.counts[:c.n])
    assert tot["split_packets"] == 0 and tot["overflow"] == 0 and out.n == b.n and frags.sum() > 500
    assert (disp[frags] == abi.FRAG_ALREADY).all() and (index == np.arange(b.n)).all() and not frag_no.any()
    assert (out.offsets == b.offsets).all() and (out.caplens == b.caplens).all()
    assert bytes(out.data) == bytes(b.data[:int(b.caplens.sum())])


# ---------------------------------------------------------------- the base scan's second step
N_WIDE, STEP = 66 * fc.BLOCK + 7, 64  # blocks a step of the base kernel takes
WIDE_TOTALS = {"out_packets": 115881, "out_bytes": 15776646, "split_packets": 8958, "fragments": 57248,
               "copied": 58633, "under_size": 53688}  # frozen; none is zero: every carried sum is used


@functools.lru_cache(maxsize=None)
def wide():
    """(the 67-block case, what the reference leaves): built once, shared by the CPU and the GPU test."""
    case = fc.make("wide", fc.mixed(np.random.default_rng(31), N_WIDE), frag_size=128)
    return case, fc.run_reference(case)


def test_reference_past_64_blocks():
    case, want = wide()
    assert case.n == N_WIDE and (N_WIDE + fc.BLOCK - 1) // fc.BLOCK == STEP + 3
    fc.assert_same(want, fc.brute(case), "wide")
    totals = abi.frag_totals_dict(want.totals)
    assert totals["overflow"] == 0 and totals["bad_desc"] == 0
    cnt = want.counts[:N_WIDE].astype(np.int64)
    split = want.disposition[:N_WIDE] == abi.FRAG_SPLIT
    for blk in (STEP, STEP + 1):  # the blocks behind the step line put packets out, fragments among them
        rows = slice(blk * fc.BLOCK, (blk + 1) * fc.BLOCK)
        assert int(cnt[rows].sum()) > fc.BLOCK and int(split[rows].sum()) >= 1, blk
    assert all(v != 0 for v in WIDE_TOTALS.values()) and {k: totals[k] for k in WIDE_TOTALS} == WIDE_TOTALS


@pytest.mark.gpu
def test_gpu_frag_past_64_blocks(engine):
    """The device equals the reference; and defrag on the device over the fragmented batch, whose groups then lie on
    both sides of the step line of defrag's own scan, equals defrag's reference."""
    case, want = wide()
    got = fc.run_device(engine, case)
    fc.assert_same(got, want, "wide")
    back = defrag_case_of(fc.output_batch(got))
    ref = dc.run_reference(back)
    t = abi.defrag_totals_dict(ref.totals)
    assert back.n == WIDE_TOTALS["out_packets"] > (STEP + 1) * dc.BLOCK and t["overflow"] == 0
    assert t["reassembled"] > 8000 and t["out_packets"] > (STEP + 1) * dc.BLOCK
    dc.assert_same(dc.run_device(engine, back), ref, "wide, defragmented")
