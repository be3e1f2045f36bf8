"""pcppx_select_device: the kept packets of a device batch gathered into a packed batch (include/pcppx.h, select).

CPU: pcppx_select_reference (the contract in plain C++ over host pointers) equals a brute-force per-packet Python
loop on every case family of tests/select_cases.py; the ctypes mirrors match the header; every bad-argument
combination is refused before any device work.
GPU: pcppx_select_device equals pcppx_select_reference byte for byte -- data, offsets, caplens, index, totals, and the
0xA5 fill of everything beyond WRITTEN_* -- on the same cases; the flags mode over a real parse's summary / brief
equals the mask mode; a parse of the selected batch equals the selected rows of the original parse; and
filter -> select -> D2H -> write_pcap writes exactly the packets the worker would send on.
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

import oracle
import select_cases as sc
from conftest import golden_files, load_golden
from pcapplusplus_amd import abi
from test_filter import OPTS as FILTER_OPTS
from test_filter import batches, device_finishable, gpu_filter, specs_for

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
CASES = sc.cases()


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    sc.assert_same(sc.run_reference(case), sc.brute(case), case.name)


def test_cases_cover_the_kernel_shapes():
    """The block size the cases are built around is the copy kernel's, and the families reach the paths they name."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kSelectBlockPk\s*=\s*(\d+)", txt).group(1)) == sc.BLOCK
    by = {c.name: c for c in CASES}
    assert max(c.n for c in CASES if c.name != "scan3") <= 100_000
    assert by[f"n{90 * sc.BLOCK + 5}"].n > 64 * sc.BLOCK  # more blocks than a wave has lanes
    assert re.search(r"\(256 per step", (abi.PKG_DIR / "csrc" / "pcppx_select.hip").read_text()) and sc.BASE_STEP == 256
    s3 = by["scan3"]  # the base scan's third step, a kept packet in it, and a batch that stays small in bytes
    assert s3.n == 2 * sc.BASE_STEP * sc.BLOCK + 1029 and -(-s3.n // sc.BLOCK) > 2 * sc.BASE_STEP
    assert 1 <= int(s3.caplens.min()) and int(s3.caplens.max()) <= 8 and s3.keep[2 * sc.BASE_STEP * sc.BLOCK:].any()
    t = sc.brute(by["cap_short1"]).totals
    sp, sb = sc.selected_totals(by["cap_exact"])  # the totals with room for everything
    assert int(t[abi.SEL_WRITTEN_PACKETS]) == sp - 1 and int(t[abi.SEL_SELECTED_PACKETS]) == sp
    assert int(sc.brute(by["cap_exact"]).totals[abi.SEL_WRITTEN_BYTES]) == sb
    assert 0 < int(sc.brute(by["cap_half"]).totals[abi.SEL_WRITTEN_PACKETS]) < sp
    assert int(sc.brute(by["bad_desc_all"]).totals[abi.SEL_BAD_DESC]) > 30
    for c in CASES:
        if c.name.startswith("start"):  # the last packet ends exactly at data_len
            assert int(c.offsets[-1]) + int(c.caplens[-1]) == c.dlen()


def test_select_structs_match_header():
    fields = {"pcppx_select_spec": abi.SelectSpec, "pcppx_selection": abi.Selection}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu\\n", sizeof(pcppx_select_spec), sizeof(pcppx_selection));\n'
           '  printf("%d %d %d %d %d %d %d\\n", PCPPX_SEL_SELECTED_PACKETS, PCPPX_SEL_SELECTED_BYTES,\n'
           '         PCPPX_SEL_WRITTEN_PACKETS, PCPPX_SEL_WRITTEN_BYTES, PCPPX_SEL_BAD_DESC, PCPPX_SEL_TOTALS,\n'
           '         PCPPX_ABI_VERSION);\n' + lines + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.SelectSpec), C.sizeof(abi.Selection)]
    assert [int(x) for x in out[1].split()] == [abi.SEL_SELECTED_PACKETS, abi.SEL_SELECTED_BYTES,
                                                abi.SEL_WRITTEN_PACKETS, abi.SEL_WRITTEN_BYTES, abi.SEL_BAD_DESC,
                                                abi.SEL_TOTALS, abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        seen += 1
    assert seen == len(abi.SelectSpec._fields_) + len(abi.Selection._fields_)
    assert abi.FLAGS_OFFSET == 12 and abi.SEL_FIELDS[abi.SEL_BAD_DESC] == "bad_desc"


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    s = abi.make_select_spec(keep=1)
    o = abi.Selection(1, 1, 1, 1, 1, 1, 0, 1)
    return b, s, o


BAD_ARGS = {
    "null_totals": lambda b, s, o: setattr(o, "totals", None),
    "null_offsets": lambda b, s, o: setattr(o, "offsets", None),
    "null_caplens": lambda b, s, o: setattr(o, "caplens", None),
    "keep_and_flags_null": lambda b, s, o: setattr(s, "keep", None),
    "keep_and_flags_set": lambda b, s, o: (setattr(s, "flags", 1), setattr(s, "flags_stride", 32)),
    "flags_stride_0": lambda b, s, o: (setattr(s, "keep", None), setattr(s, "flags", 1), setattr(s, "flags_stride", 0)),
    "flags_stride_8": lambda b, s, o: (setattr(s, "keep", None), setattr(s, "flags", 1), setattr(s, "flags_stride", 8)),
    "flags_stride_24": lambda b, s, o: (setattr(s, "keep", None), setattr(s, "flags", 1),
                                        setattr(s, "flags_stride", 24)),
    "flags_stride_64": lambda b, s, o: (setattr(s, "keep", None), setattr(s, "flags", 1),
                                        setattr(s, "flags_stride", 64)),
    "spec_reserved": lambda b, s, o: setattr(s, "reserved", 1),
    "spec_reserved2": lambda b, s, o: setattr(s, "reserved2", 1),
    "out_reserved": lambda b, s, o: setattr(o, "reserved", 1),
}


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_select_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    lib = abi.load_engine()
    ctx = C.c_void_p(1)
    b, s, o = _good_args()
    BAD_ARGS[what](b, s, o)
    assert lib.pcppx_select_device(ctx, C.byref(b), C.byref(s), C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_select_reference(C.byref(b), C.byref(s), C.byref(o)) == abi.E_INVAL


def test_select_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    ctx = C.c_void_p(1)
    b, s, o = _good_args()
    assert lib.pcppx_select_device(None, C.byref(b), C.byref(s), C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_select_device(ctx, None, C.byref(s), C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_select_device(ctx, C.byref(b), None, C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_select_device(ctx, C.byref(b), C.byref(s), None, None) == abi.E_INVAL
    assert lib.pcppx_select_reference(None, C.byref(s), C.byref(o)) == abi.E_INVAL
    assert lib.pcppx_select_reference(C.byref(b), None, C.byref(o)) == abi.E_INVAL
    assert lib.pcppx_select_reference(C.byref(b), C.byref(s), None) == abi.E_INVAL
    # the flags mode with either legal stride, and an empty batch, pass the checks (reference: no context needed)
    for stride in (16, 32):
        c = next(x for x in CASES if x.name == f"flags_stride{stride}")
        assert int(sc.run_reference(c).totals[abi.SEL_SELECTED_PACKETS]) > 0
    empty = sc.run_reference(next(x for x in CASES if x.name == "n0"))
    assert list(empty.totals) == [0] * abi.SEL_TOTALS


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_select_equals_reference(engine, case):
    sc.assert_same(sc.run_device(engine, case), sc.run_reference(case), case.name)


def _golden(stem):
    return load_golden(next(p for p in golden_files() if p.stem == stem))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("stem", ["synth_cfg3", "pcap_lt1"])
def test_gpu_select_flags_mode_over_a_real_parse(engine, stem):
    """flags_any = PCPPX_F_NEEDS_HOST through the summary (stride 32) and the brief (stride 16) a device parse wrote:
    the hand-off list of the packets the host must finish. Equals the mask mode with the mask computed on the host."""
    from pcapplusplus_amd.engine import parse_on_device_ex, select_on_device

    b = _golden(stem)
    rec = parse_on_device_ex(engine, b, abi.make_opts(), brief=True)
    # the clean synthetic set has no NEEDS_HOST packet (an empty hand-off list); a second mask selects part of each set
    for any_ in (abi.F_NEEDS_HOST, abi.F_L4_CSUM_OK | abi.F_TRAILER):
        needs = (rec["summary"]["flags"] & any_) != 0
        assert not needs.all() and (needs.any() or (stem, any_) == ("synth_cfg3", abi.F_NEEDS_HOST))
        want = sc.run_reference(sc.Case(stem, b.data, b.offsets, b.caplens, keep=needs.astype(np.uint8)))
        for records in (rec["summary"], rec["brief"]):
            case = sc.Case(stem, b.data, b.offsets, b.caplens, flags=np.ascontiguousarray(records).view(np.uint8),
                           flags_stride=records.dtype.itemsize, flags_any=any_)
            sc.assert_same(sc.run_device(engine, case), want, f"{stem} stride {case.flags_stride}")
            got, index, tot = select_on_device(engine, b, flags=records, flags_any=any_, index_only=True)
            assert np.array_equal(index, np.nonzero(needs)[0]) and tot["written_packets"] == int(needs.sum())
            assert np.array_equal(got.caplens, b.caplens[needs])


@pytest.mark.gpu
@pytest.mark.parametrize("name,batch", batches(), ids=lambda x: x if isinstance(x, str) else "")
def test_gpu_select_closure_under_parse(engine, name, batch):
    """The output is an ordinary batch: its device parse equals rows `index` of the source batch's device parse, and
    the restatement's parse of it."""
    from pcapplusplus_amd.engine import parse_on_device, select_on_device

    opts = abi.make_opts()
    keep = (np.random.default_rng(11).random(batch.n) < 0.5).astype(np.uint8)
    sub, index, tot = select_on_device(engine, batch, keep=keep)
    assert np.array_equal(index, np.nonzero(keep)[0]) and tot["bad_desc"] == 0
    assert tot["written_packets"] == tot["selected_packets"] == int(keep.sum())
    fsum, flay = parse_on_device(engine, batch, opts)
    ssum, slay = parse_on_device(engine, sub, opts)
    oracle.compare_exact(ssum, slay, fsum[index], flay[index])
    osum, olay = oracle.oracle_parse(sub, opts)
    oracle.compare_exact(ssum, slay, osum, olay)


@pytest.mark.gpu
@pytest.mark.parametrize("name,batch", batches(), ids=lambda x: x if isinstance(x, str) else "")
def test_gpu_filter_select_write_pcap(engine, name, batch, tmp_path):
    """The worker's send-on step: filter -> select by matched[] -> D2H -> write_pcap. The file holds exactly the
    packets the worker (the restatement, and the reference where it is built) matches, in order."""
    from pcapplusplus_amd.engine import PcapReader, select_on_device
    from pcapplusplus_amd.pcap import write_pcap

    b = device_finishable(batch)
    b.timestamps_ns = (np.arange(b.n, dtype=np.uint64) + 1) * np.uint64(1_000_000)
    b.frame_lens = b.caplens + np.uint32(4)
    s, lay = oracle.oracle_parse(b, FILTER_OPTS)
    specs = specs_for(b, 1)
    sent = 0
    for k in (1, 3, len(specs) - 1):  # a protocol, a spec drawn from the batch, and one that may match nothing
        spec = specs[k]
        matched, _ = gpu_filter(engine, b, spec)
        sub, index, tot = select_on_device(engine, b, keep=matched)
        want = np.nonzero(oracle.oracle_filter(b, s, lay, spec)[0])[0]
        assert np.array_equal(index, want), (name, k)
        sent += len(want)
        if oracle.ref_available():
            assert np.array_equal(index, np.nonzero(oracle.ref_filter(b, spec)[0])[0]), (name, k)
        path = tmp_path / f"{name}_{k}.pcap"
        write_pcap(path, sub)
        with PcapReader(str(path)) as rd:
            back = rd.read_batch(max_packets=max(len(want), 1) + 1, data_cap=int(tot["written_bytes"]) + 64)
        assert back.n == len(want) and back.linktype == b.linktype
        assert np.array_equal(back.caplens, b.caplens[want])
        assert np.array_equal(back.timestamps_ns, b.timestamps_ns[want])
        assert np.array_equal(back.frame_lens, b.frame_lens[want])
        assert back.data[: int(back.caplens.sum())].tobytes() == b"".join(b.packet(int(i)) for i in want), (name, k)
    assert sent > 0, name
