"""pcppx_tcpstream_device: the TCP connection sides that are clean inside one device batch (include/pcppx.h, tcpstream).

CPU: the ctypes mirrors match the header and every bad-argument combination is refused before any device work;
pcppx_tcpstream_reference (the contract in plain C++ over host pointers) equals a brute-force Python restatement of the
contract on every case family of tests/tcpstream_cases.py, byte for byte, the 0xA5 fill of everything else included
(all of it but the totals on overflow); a second model, TcpReassembly::reassemblePacket restated as a streaming machine
(pcapplusplus_amd.tcpstream.Reassembler), reproduces the reference's own test vectors (tests/golden/tcpstream: data
files of Tests/Pcap++Test/PcapExamples); and on every case, under both base_clear values, every side the contract
calls clean is delivered by that machine as exactly the stream the contract puts out: no marker, no trimmed piece.
The reference runs under ASan + UBSan in a stand-alone program.
GPU: pcppx_tcpstream_device equals pcppx_tcpstream_reference byte for byte on the same cases; two calls on two streams
agree and a repeat is bit-identical; source packets on both sides of offset 2^32; sessions -> parse + reasm ->
tcpstream gives the generator's plaintext; the reference's vectors on the device.
"""
from __future__ import annotations

import ctypes as C
import re
import shutil
import subprocess
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import tcpstream_cases as tc
from conftest import GOLDEN
from pcapplusplus_amd import abi
from pcapplusplus_amd import tcpstream as ts
from pcapplusplus_amd.pcap import read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "tcpstream"
CASES = tc.cases()
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if c.n <= 5100]


# ---------------------------------------------------------------- CPU: the ABI
def test_tcpstream_structs_match_header():
    fields = {"pcppx_tcpstream_spec": abi.TcpStreamSpec, "pcppx_tcpstreams": abi.TcpStreams}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    lines += "".join(f'  printf("rec.{f} %zu %zu\\n", offsetof(pcppx_tcpstream_rec, {f}), '
                     f'sizeof(((pcppx_tcpstream_rec*)0)->{f}));\n' for f in abi.TCPSTREAM_DTYPE.names)
    consts = ["PCPPX_TCPS_F_SYN", "PCPPX_TCPS_F_FIN", "PCPPX_TCPS_F_RST", "PCPPX_TCPS_F_OOO", "PCPPX_TCPS_NOT_TCP",
              "PCPPX_TCPS_HOST", "PCPPX_TCPS_LEFT", "PCPPX_TCPS_STREAM", "PCPPX_TCPS_CONTROL", "PCPPX_TCPS_BAD_DESC",
              "PCPPX_TCPS_STREAMS", "PCPPX_TCPS_BYTES", "PCPPX_TCPS_SEGMENTS", "PCPPX_TCPS_LEFT_N",
              "PCPPX_TCPS_CANDIDATES", "PCPPX_TCPS_HOST_N", "PCPPX_TCPS_BAD_DESC_N", "PCPPX_TCPS_OVERFLOW",
              "PCPPX_TCPS_TOTALS", "PCPPX_ABI_VERSION"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %u\\n", sizeof(pcppx_tcpstream_spec), sizeof(pcppx_tcpstreams), '
           'sizeof(pcppx_tcpstream_rec), PCPPX_TCPS_NONE);\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.TcpStreamSpec), C.sizeof(abi.TcpStreams),
                                                abi.TCPSTREAM_DTYPE.itemsize, abi.TCPS_NONE]
    assert [int(x) for x in out[1].split()] == [
        abi.TCPS_F_SYN, abi.TCPS_F_FIN, abi.TCPS_F_RST, abi.TCPS_F_OOO, abi.TCPS_NOT_TCP, abi.TCPS_HOST, abi.TCPS_LEFT,
        abi.TCPS_STREAM, abi.TCPS_CONTROL, abi.TCPS_BAD_DESC, abi.TCPS_STREAMS, abi.TCPS_BYTES, abi.TCPS_SEGMENTS,
        abi.TCPS_LEFT_N, abi.TCPS_CANDIDATES, abi.TCPS_HOST_N, abi.TCPS_BAD_DESC_N, abi.TCPS_OVERFLOW, abi.TCPS_TOTALS,
        abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        if t == "rec":
            ft, fo = abi.TCPSTREAM_DTYPE.fields[f][:2]
            assert (fo, ft.itemsize) == (int(off), int(size)), name
        else:
            d = getattr(fields[t], f)
            assert (d.offset, d.size) == (int(off), int(size)), name
        seen += 1
    assert seen == len(abi.TcpStreamSpec._fields_) + len(abi.TcpStreams._fields_) + len(abi.TCPSTREAM_DTYPE.names)
    assert abi.ABI_VERSION == 7 and len(abi.TCPS_FIELDS) == abi.TCPS_TOTALS


def test_tcpstream_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_tcpstream_device", "pcppx_tcpstream_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_tcpstream_spec(True, 0)
    o = abi.TcpStreams(1, 1, 1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, info=1, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _spec_reserved(a, k):
    a["s"].reserved[k] = 1


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_streams": lambda a: _set(a, "o", "streams", None),
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
    "max_layers_255": lambda a: a.update(ml=255),
    "base_clear_2": lambda a: _set(a, "s", "base_clear", 2),
    "spec_reserved_0": lambda a: _spec_reserved(a, 0),
    "spec_reserved_2": lambda a: _spec_reserved(a, 2),
    "out_reserved": lambda a: _set(a, "o", "reserved", 1),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_tcpstream_device's, pcppx_tcpstream_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_tcpstream_device(ctx, ref("b"), ref("r"), a["ml"], a["info"], ref("s"), ref("o"), None)
    host = None if ctx is None else \
        lib.pcppx_tcpstream_reference(ref("b"), ref("r"), a["ml"], a["info"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_tcpstream_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_tcpstream_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # a brief instead of the summary, the optional columns absent and an empty batch without info pass the checks
    for name in ("brief", "no_columns", "n0"):
        assert int(tc.run_reference(BY_NAME[name]).totals[abi.TCPS_OVERFLOW]) == 0
    empty = tc.run_reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.TCPS_TOTALS
    tc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    got = tc.run_reference(case)
    tc.assert_same(got, tc.brute(case), case.name)
    if case.name in tc.OVERFLOWING:
        assert int(got.totals[abi.TCPS_OVERFLOW]) == 1
        tc.assert_untouched(got, case.name)
    elif case.name in tc.EXPECT:  # what the family was built to show
        t = abi.tcpstream_totals_dict(got.totals)
        assert (t["streams"], t["left"]) == tc.EXPECT[case.name], (case.name, t)


def test_cases_cover_the_kernel_shapes():
    """The block size the cases are built around is the kernels', and the families reach the paths they name."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kTcpsBlockPk\s*=\s*(\d+)", txt).group(1)) == tc.BLOCK
    assert max(c.n for c in CASES) <= 70_000 and BY_NAME["big"].n > 64 * tc.BLOCK
    assert sum(c.n > 5100 for c in CASES) == 1
    for name in tc.OVERFLOWING:
        assert int(tc.brute(BY_NAME[name]).totals[abi.TCPS_OVERFLOW]) == 1, name
    ns, nb, nc = tc.output_totals(BY_NAME["plain"])
    exact = abi.tcpstream_totals_dict(tc.brute(BY_NAME["cap_exact"]).totals)
    assert (exact["streams"], exact["bytes"], exact["candidates"], exact["overflow"]) == (ns, nb, nc, 0)
    got = tc.brute(BY_NAME["elephant_late_segment"])
    (r,) = got.records()
    assert int(r["segments"]) == 5000 and int(r["flags"]) & abi.TCPS_F_OOO
    assert not int(tc.brute(BY_NAME["elephant"]).records()[0]["flags"]) & abi.TCPS_F_OOO
    for n in (tc.BLOCK - 1, tc.BLOCK, tc.BLOCK + 1):  # the members of a side in two blocks and several tiles
        d = tc.brute(BY_NAME[f"blocks_n{n}"]).disposition[:n + 72]
        members = np.nonzero((d == abi.TCPS_STREAM) | (d == abi.TCPS_CONTROL))[0]
        assert len({int(j) // tc.BLOCK for j in members}) == 2 and len({int(j) // 64 for j in members}) >= 4
    t = abi.tcpstream_totals_dict(tc.brute(BY_NAME["bad_desc"]).totals)
    assert t["bad_desc"] > 20 and t["streams"] > 20 and t["left"] > 0
    t = abi.tcpstream_totals_dict(tc.brute(BY_NAME["mixed"]).totals)
    assert t["host"] == 8 and t["streams"] > 20
    got = tc.brute(BY_NAME["seq_wrap"])
    first = [int(r["first"]) for r in got.records()]
    c = BY_NAME["seq_wrap"]
    seqs = [g.seq for k, g in ts.candidates(c.batch(), c.summary, c.layers, c.info) if g is not None and g.len]
    assert len(first) == 2 and min(seqs) < 100 and max(seqs) > 0xFFFFFF00  # the numbers wrap inside a stream
    pos = {(int(c.offsets[i]) + g.pay) % 16 for c in (BY_NAME["alignments_0"],)
           for i, (k, g) in enumerate(ts.candidates(c.batch(), c.summary, c.layers, c.info)) if g is not None and g.len}
    got = tc.brute(BY_NAME["alignments_0"])
    dst = {(int(got.records()[int(s)]["pos"]) + int(p)) % 16
           for s, p, d in zip(got.seg_stream, got.seg_pos, got.disposition) if d == abi.TCPS_STREAM}
    assert pos == set(range(16)) and dst == set(range(16))
    fams = {g.src[0] for c in (BY_NAME["ipv6"], BY_NAME["plain"])
            for k, g in ts.candidates(c.batch(), c.summary, c.layers, c.info) if g is not None}
    assert fams == {4, 6}


def test_default_mix_reassembles_at_least_half_of_its_sides():
    """A condition on the generator, checked by the brute-force model: the property tests below do not pass by
    reassembling nothing."""
    for name in ("sessions_bc1", "sessions_bc0", "sessions_v6_vlan"):
        c = BY_NAME[name]
        sides = {(g.key, g.src) for k, g in ts.candidates(c.batch(), c.summary, c.layers, c.info) if g is not None}
        t = abi.tcpstream_totals_dict(tc.brute(c).totals)
        assert t["streams"] * 2 >= len(sides) and t["left"] > 0, (name, t, len(sides))


# ---------------------------------------------------------------- CPU: the streaming model against the reference's data
def vector_case(name: str, **kw) -> tc.Case:
    return tc.parsed(name, read_pcap(VECTORS / name), **kw)


def machine_over(c: tc.Case, base_clear: bool = True) -> ts.Reassembler:
    m = ts.Reassembler(base_clear)
    m.feed_batch(c.batch(), c.summary, c.layers, c.info)
    return m


def _port(src: bytes) -> int:
    return int.from_bytes(src[1:3], "big")


def test_stream_model_reproduces_the_reference_vectors():
    """What the reference's tests expect (Tests/Pcap++Test/Tests/TcpReassemblyTests.cpp): the callbacks' data in the
    order they come, per connection for three_http_streams."""
    c = vector_case("three_http_streams.pcap")
    m = machine_over(c)
    m.close_all()
    by_port = {_port(m.sides_of(key)[0]): key for key in m.conns}
    for k, (port, size) in enumerate(((44305, 1005), (52328, 1112), (54615, 818)), 1):
        key = by_port[port]
        text = b"".join(d for kk, _, d in m.log if kk == key)
        assert len(text) == size and text == (VECTORS / f"three_http_streams_conn_{k}_output.txt").read_bytes()
        assert text == m.stream(key, 0) + m.stream(key, 1)  # the request, then the response
    for name, sizes in (("one_http_stream_fin", (367, 3549)), ("one_http_stream_fin2", (406, 7071)),
                        ("one_tcp_stream", (9948, 12444))):
        m = machine_over(vector_case(name + ".pcap"))
        m.close_all()
        (key,) = m.conns
        assert b"".join(d for _, _, d in m.log) == (VECTORS / f"{name}_output.txt").read_bytes(), name
        assert (len(m.stream(key, 0)), len(m.stream(key, 1))) == sizes
    m = machine_over(vector_case("unidirectional_tcp_stream_with_missing_packet.pcap"))
    m.close_all()
    (key,) = m.conns
    assert [x[1] for x in m.messages[(key, 0)] if x[1]] == [1420] and b"[1420 bytes missing]" in m.stream(key, 0)


def test_reference_on_the_vectors():
    c = vector_case("three_http_streams.pcap")
    got = tc.run_reference(c)
    recs = got.records()
    assert len(recs) == 6 and not (recs["flags"] & abi.TCPS_F_OOO).any() and int(got.totals[abi.TCPS_LEFT_N]) == 0
    kinds = ts.candidates(c.batch(), c.summary, c.layers, c.info)
    for k, (port, size) in enumerate(((44305, 1005), (52328, 1112), (54615, 818)), 1):
        (j,) = [j for j, r in enumerate(recs) if r["side"] == 0 and _port(kinds[int(r["first"])][1].src) == port]
        text = got.stream(j) + got.stream(int(recs[j]["peer"]))
        assert len(text) == size and text == (VECTORS / f"three_http_streams_conn_{k}_output.txt").read_bytes()
    for name, sizes in (("one_http_stream_fin", (367, 3549)), ("one_http_stream_fin2", (406, 7071))):
        got = tc.run_reference(vector_case(name + ".pcap"))
        assert [int(b) for b in got.records()["bytes"]] == list(sizes)
        assert got.stream(0) + got.stream(1) == (VECTORS / f"{name}_output.txt").read_bytes()
    c = vector_case("one_tcp_stream.pcap")
    got = tc.run_reference(c)
    (r,) = got.records()  # 80 -> 61541 is clean; 61541 -> 80 does not tile and is LEFT
    assert (int(r["bytes"]), int(r["side"]), int(r["peer"])) == (12444, 1, abi.TCPS_NONE)
    assert _port(ts.candidates(c.batch(), c.summary, c.layers, c.info)[int(r["first"])][1].src) == 80
    m = machine_over(c)
    assert got.stream(0) == m.stream(int(r["flow_key"]), 1)
    done = ts.complete_on_host(c.batch(), c.summary, c.layers, c.info, got.disposition[:c.n])
    assert done.stream(int(r["flow_key"]), 0) == m.stream(int(r["flow_key"]), 0)  # the LEFT side, finished on the host
    got = tc.run_reference(vector_case("unidirectional_tcp_stream_with_missing_packet.pcap"))
    assert int(got.totals[abi.TCPS_STREAMS]) == 0 and int(got.totals[abi.TCPS_LEFT_N]) == int(got.totals[abi.TCPS_CANDIDATES]) > 0


# ---------------------------------------------------------------- CPU: soundness
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_clean_sides_are_what_the_stream_delivers(case):
    """Under both switches: every side the contract calls clean has, as the concatenation of the machine's callbacks
    for it, exactly the stream the contract puts out, without a marker or a trimmed piece."""
    if not case.want_columns or case.index_only or case.name in tc.OVERFLOWING:
        case = replace(case, want_columns=True, index_only=False, data_cap=None, max_packets=None, max_segments=0)
    for bc in (True, False):
        c = replace(case, base_clear=bc)
        got = tc.run_reference(c)
        m = machine_over(c, bc)  # no close: a clean side needs none
        for j, r in enumerate(got.records()):
            msgs = m.messages.get((int(r["flow_key"]), int(r["side"])), [])
            assert not any(x[1] or x[2] for x in msgs), (case.name, bc, j)
            assert b"".join(x[0] for x in msgs) == got.stream(j), (case.name, bc, j)
            assert len(msgs) == int(r["segments"])  # each data member's whole payload, once


def test_sessions_plaintext_through_the_reference():
    s = ts.sessions(40, (1, 6), mss=300, seed=21, ipv6=0.3, **tc.DEFAULT_MIX)
    c = tc.parsed("sessions", s.batch)
    got = tc.run_reference(c)
    recs = got.records()
    assert len(recs) >= 40
    for j, r in enumerate(recs):
        f = int(r["first"])
        assert got.stream(j) == s.plaintext(int(s.conn[f]), int(s.side[f])), j


def test_left_packets_complete_on_the_host():
    """The sides the contract reassembles and the sides the host machine gets from the LEFT packets are, together,
    the sides TcpReassembly delivers data for over the whole batch; none is delivered twice."""
    s = ts.sessions(120, (1, 8), mss=300, seed=22, ipv6=0.3, **tc.DEFAULT_MIX)
    c = tc.parsed("sessions", s.batch)
    got = tc.run_reference(c)
    kinds = ts.candidates(c.batch(), c.summary, c.layers, c.info)
    named = lambda m: {(key, m.sides_of(key)[side]) for key, side in m.messages}  # noqa: E731
    dev = {(int(r["flow_key"]), kinds[int(r["first"])][1].src) for r in got.records()}
    done = ts.complete_on_host(c.batch(), c.summary, c.layers, c.info, got.disposition[:c.n])
    whole = machine_over(c)
    assert len(dev) >= 120 and len(named(done)) >= 10
    assert dev.isdisjoint(named(done)) and dev | named(done) == named(whole)


def test_reference_under_sanitizers(tmp_path):
    """pcppx_tcpstream_reference in a stand-alone program (its own main, host compiler, no HIP, nothing loaded into
    python) built with ASan + UBSan, over three cases in exact-size heap buffers; the results equal the brute force's."""
    gxx = shutil.which("g++")
    assert gxx is not None
    exe = tmp_path / "tcpstream_ref_check"
    csrc = abi.PKG_DIR / "csrc"
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), str(abi.REPO_DIR / "tests" / "native" / "tcpstream_ref_check.cpp"),
                    str(csrc / "pcppx_tcpstream_ref.cpp"), "-o", str(exe)], check=True)
    files = []
    for name in ("sessions_bc1", "bad_desc", "records_outside", "index_only", "cap_short1", "brief"):
        c = BY_NAME[name]
        want = tc.brute(c)
        rec = c.summary
        if c.use_brief:
            rec = np.zeros(c.n, abi.BRIEF_DTYPE)
            for f in abi.BRIEF_DTYPE.names:
                rec[f] = c.summary[f]
        head = np.array([c.n, c.dlen(), tc.ML, 0 if c.use_brief else 1, int(c.base_clear), c.max_segments, c.maxp(),
                         c.cap(), int(c.index_only), int(c.want_columns), len(want.streams),
                         0 if want.data is None else len(want.data)], np.uint64)
        parts = [head, c.data[:c.dlen()], c.offsets, c.caplens, rec, c.layers, c.info, want.streams]
        parts += [want.disposition, want.seg_stream, want.seg_pos] if c.want_columns else []
        parts += [] if want.data is None else [want.data]
        parts.append(want.totals)
        path = tmp_path / f"{name}.case"
        path.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))
        files.append(str(path))
    env = {"TMPDIR": str(tmp_path), "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count("equal") == len(files)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_tcpstream_equals_reference(engine, case):
    want = tc.run_reference(case)
    got = tc.run_device(engine, case)
    tc.assert_same(got, want, case.name)
    if case.name in tc.OVERFLOWING:
        tc.assert_untouched(got, case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sessions_bc1", "elephant_late_segment", "big", "maxseg_short1", "overlapping"])
def test_gpu_tcpstream_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = tc.run_reference(case)
    runs = [tc.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        tc.assert_same(r.result(), want, f"{name} run {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 9])
def test_gpu_tcpstream_source_on_both_sides_of_4gib(engine, mis):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32:
    one packet lies across each line, members of one side on both sides."""
    import torch

    import wide_cases as wc

    case = replace(BY_NAME["plain"], out_misalign=3)
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
    wide = replace(case, offsets=offs.astype(np.uint64))
    source = (data, torch.from_numpy(wide.offsets.view(np.int64)).to("cuda:0"),
              torch.from_numpy(wide.caplens.view(np.int32)).to("cuda:0"), lay.data_len)
    want = tc.run_reference(case)
    assert int(want.totals[abi.TCPS_STREAMS]) == 30
    member = want.disposition[:n] == abi.TCPS_STREAM
    assert any(len({bool(wide.offsets[j] < wc.LINE) for j in np.nonzero(member & (want.seg_stream[:n] == s))[0]}) == 2
               for s in range(30))
    got = tc.run_device(engine, case, source=source)
    tc.assert_same(got, want, f"wide mis{mis}")
    del raw, data, source
    torch.cuda.empty_cache()


def _device_parse_reasm(engine, batch, opts):
    import torch

    from pcapplusplus_amd.engine import to_device

    data, offsets, caplens = to_device(batch)
    n = batch.n
    summary = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    layers = torch.zeros(n * opts.max_layers * 8, dtype=torch.uint8, device="cuda:0")
    info = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    engine.parse_reasm_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, info,
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (summary.cpu().numpy().view(abi.SUMMARY_DTYPE), layers.cpu().numpy().view(abi.LAYER_DTYPE).reshape(n, -1),
            info.cpu().numpy().view(abi.REASM_DTYPE))


@pytest.mark.gpu
def test_gpu_sessions_parse_tcpstream_end_to_end(engine):
    from pcapplusplus_amd.engine import tcpstream_on_device

    s = ts.sessions(300, (1, 8), mss=700, seed=31, ipv6=0.3, **tc.DEFAULT_MIX)
    summary, layers, info = _device_parse_reasm(engine, s.batch, tc.OPTS)
    data, recs, disp, seg_stream, seg_pos, tot = tcpstream_on_device(engine, s.batch, summary, layers, info)
    assert tot["overflow"] == 0 and tot["host"] == 0 and tot["streams"] == len(recs) >= 300 and tot["left"] > 0
    for r in recs:
        f = int(r["first"])
        assert data[int(r["pos"]):int(r["pos"]) + int(r["bytes"])].tobytes() == \
            s.plaintext(int(s.conn[f]), int(s.side[f])), f
    # the batch of the benchmark's generator: every side clean and in order
    b, side = ts.session_batch(20000, 500, seed=5)
    summary, layers, info = _device_parse_reasm(engine, b, tc.OPTS)
    data, recs, disp, seg_stream, seg_pos, tot = tcpstream_on_device(engine, b, summary, layers, info)
    assert tot["segments"] == tot["candidates"] == b.n and tot["bytes"] == int(b.caplens.sum()) - 54 * b.n
    assert not (recs["flags"] & abi.TCPS_F_OOO).any() and tot["streams"] == len(np.unique(side))


@pytest.mark.gpu
def test_gpu_tcpstream_on_the_reference_vectors(engine):
    from pcapplusplus_amd.engine import tcpstream_on_device

    for name in ("three_http_streams.pcap", "one_http_stream_fin.pcap", "one_http_stream_fin2.pcap",
                 "one_tcp_stream.pcap", "unidirectional_tcp_stream_with_missing_packet.pcap"):
        c = vector_case(name)
        tc.assert_same(tc.run_device(engine, c), tc.run_reference(c), name)
    b = read_pcap(VECTORS / "one_http_stream_fin2.pcap")
    summary, layers, info = _device_parse_reasm(engine, b, tc.OPTS)
    data, recs, disp, seg_stream, seg_pos, tot = tcpstream_on_device(engine, b, summary, layers, info)
    assert [int(x) for x in recs["bytes"]] == [406, 7071] and [int(x) for x in recs["peer"]] == [1, 0]
    assert data.tobytes() == (VECTORS / "one_http_stream_fin2_output.txt").read_bytes()
