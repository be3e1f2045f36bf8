"""pcppx_tlsfp_device: JA3 / JA3S fingerprints of the TLS hellos of a device batch (include/pcppx.h, tlsfp).

CPU: the ctypes mirrors match the header and every bad-argument combination is refused before any device work;
pcppx_tlsfp_reference (the contract in plain C++ over host pointers) equals pcapplusplus_amd.tlsfp.model (the contract
in plain Python with hashlib.md5) on every case family of tests/tlsfp_cases.py, byte for byte, the 0xA5 fill of
everything else included (all of it but the totals on overflow); it reproduces the reference's own TLSFingerprinting
output files (tests/golden/tlsfp) and agrees with the model on the bundled TLS captures; its MD5 equals hashlib's on
every length 0..130; and it runs clean under ASan + UBSan in a stand-alone program.
GPU: pcppx_tlsfp_device equals pcppx_tlsfp_reference byte for byte on the same cases; two calls on two streams agree and
a repeat is bit-identical; hello packets on both sides of offset 2^32; the golden files from a device parse, through the
library and through tools/tlsfp_file.py; the records' MD5 words as pcppx_steer_device's key column; a batch of more
blocks than one step of the base scan takes.
"""
from __future__ import annotations

import ctypes as C
import functools
import hashlib
import ipaddress
import re
import shutil
import subprocess
import sys
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import oracle
import tlsfp_cases as tc
from conftest import GOLDEN
from pcapplusplus_amd import abi
from pcapplusplus_amd import tlsfp as tf
from pcapplusplus_amd.pcap import PacketBatch, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
FILES = GOLDEN / "ingest" / "files"
VECTORS = GOLDEN / "tlsfp"
CASES = tc.cases()
BY_NAME = {c.name: c for c in CASES}
KINDS = {"ch": (True, False), "sh": (False, True), "ch_sh": (True, True)}
ROWS = {"ch": 323, "sh": 302, "ch_sh": 625}
CAPTURES = ("tls_grease", "tls_zero_size_ext", "tls_server_hello", "tls1_3", "SSL-ClientHello1")


# ---------------------------------------------------------------- CPU: the ABI
def test_tlsfp_structs_match_header():
    fields = {"pcppx_tlsfp_spec": abi.TlsfpSpec, "pcppx_tlsfp_rec": abi.TlsfpRec, "pcppx_tlsfps": abi.Tlsfps}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = ["PCPPX_TLSFP_NONE", "PCPPX_TLSFP_CLIENT", "PCPPX_TLSFP_SERVER", "PCPPX_TLSFP_HOST", "PCPPX_TLSFP_BAD_DESC",
              "PCPPX_TLSFP_CLIENT_N", "PCPPX_TLSFP_SERVER_N", "PCPPX_TLSFP_TEXT_BYTES", "PCPPX_TLSFP_HOST_N",
              "PCPPX_TLSFP_BAD_DESC_N", "PCPPX_TLSFP_CANDIDATES", "PCPPX_TLSFP_OVERFLOW", "PCPPX_TLSFP_TOTALS",
              "PCPPX_ABI_VERSION"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu\\n", sizeof(pcppx_tlsfp_spec), sizeof(pcppx_tlsfp_rec), sizeof(pcppx_tlsfps));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.TlsfpSpec), C.sizeof(abi.TlsfpRec), C.sizeof(abi.Tlsfps)]
    assert [int(x) for x in out[1].split()] == [
        abi.TLSFP_NONE, abi.TLSFP_CLIENT, abi.TLSFP_SERVER, abi.TLSFP_HOST, abi.TLSFP_BAD_DESC, abi.TLSFP_CLIENT_N,
        abi.TLSFP_SERVER_N, abi.TLSFP_TEXT_BYTES, abi.TLSFP_HOST_N, abi.TLSFP_BAD_DESC_N, abi.TLSFP_CANDIDATES,
        abi.TLSFP_OVERFLOW, abi.TLSFP_TOTALS, abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        if t == "pcppx_tlsfp_rec":  # the numpy mirror too
            dt, at = abi.TLSFP_REC_DTYPE.fields[f][:2]
            assert (at, dt.itemsize) == (int(off), int(size)), name
        seen += 1
    assert seen == sum(len(cls._fields_) for cls in fields.values())
    assert abi.TLSFP_REC_DTYPE.itemsize == C.sizeof(abi.TlsfpRec) == 40
    assert abi.ABI_VERSION == 7 and len(abi.TLSFP_FIELDS) == abi.TLSFP_TOTALS


def test_tlsfp_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_tlsfp_device", "pcppx_tlsfp_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_tlsfp_spec(True, True)
    o = abi.Tlsfps(1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _kinds(a, client, server):
    a["s"].client, a["s"].server = client, server


def _spec_reserved(a, k):
    a["s"].reserved[k] = 1


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_recs": lambda a: _set(a, "o", "recs", None),
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
    "neither_kind": lambda a: _kinds(a, 0, 0),
    "client_2": lambda a: _kinds(a, 2, 0),
    "server_2": lambda a: _kinds(a, 1, 2),
    "server_255": lambda a: _kinds(a, 0, 255),
    "spec_reserved_0": lambda a: _spec_reserved(a, 0),
    "spec_reserved_1": lambda a: _spec_reserved(a, 1),
    "out_reserved": lambda a: _set(a, "o", "reserved", 1),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_tlsfp_device's, pcppx_tlsfp_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_tlsfp_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_tlsfp_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_tlsfp_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_tlsfp_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # each single kind, a brief instead of the summary, absent optional outputs and an empty batch pass
    for name in ("kinds_ch", "kinds_sh", "n63_brief", "cap_no_text_no_disp", "n0"):
        assert int(tc.run_reference(BY_NAME[name]).totals[abi.TLSFP_OVERFLOW]) == 0
    empty = tc.run_reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.TLSFP_TOTALS
    tc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_the_model(case):
    got = tc.run_reference(case)
    tc.assert_same(got, tc.model(case), case.name)
    if case.name in tc.OVERFLOWING:
        assert int(got.totals[abi.TLSFP_OVERFLOW]) == 1
        tc.assert_untouched(got, case.name)
    else:
        assert int(got.totals[abi.TLSFP_OVERFLOW]) == 0


def _texts(name: str, **kw) -> list:
    """Per packet of a case: its fingerprint text, or its disposition where it has none."""
    c = replace(BY_NAME[name], **kw)
    got = tc.run_reference(c)
    k = int(got.totals[abi.TLSFP_CANDIDATES])
    out = [int(d) for d in got.disposition[:c.n]]
    for r in got.records(k):
        pos = int(r["text_pos"])
        out[int(r["index"])] = bytes(got.text[pos:pos + int(r["text_len"])]).decode()
        assert bytes(r["md5"]) == hashlib.md5(out[int(r["index"])].encode()).digest()
        assert int(r["kind"]) == int(got.disposition[int(r["index"])]) and not r["reserved"].any()
    return out


CH_TEXT = "771,4865-4866-49199-156-10,0-23-10-11-65281-43,29-23-24,0-1-2"
SH_TEXT = "771,49199,65281-11-23"


def test_cases_cover_the_contract():
    """The block size the cases are built around is the kernels', and the families reach the paths they name: the
    texts here are worked out by hand from the rules of include/pcppx.h."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kTlsfpBlockPk\s*=\s*(\d+)", txt).group(1)) == tc.BLOCK
    assert max(c.n for c in CASES) <= 2100
    N, HO, BD = tc.NONE, tc.HOST, tc.BAD
    # message order, under the three settings
    both = _texts("order")
    assert both == [CH_TEXT, SH_TEXT, CH_TEXT, CH_TEXT, CH_TEXT, N, CH_TEXT, SH_TEXT, N, N, N]
    assert _texts("order", server=False) == [CH_TEXT, N, CH_TEXT, CH_TEXT, CH_TEXT, N, CH_TEXT, N, N, N, N]
    assert _texts("order", client=False) == [N, SH_TEXT, SH_TEXT, SH_TEXT, SH_TEXT, N, N, SH_TEXT, N, N, N]
    # the layers a small max_layers cuts off
    assert set(_texts("max_layers_1")) == {HO}
    assert _texts("max_layers_4") == [CH_TEXT, SH_TEXT, CH_TEXT, CH_TEXT, CH_TEXT, N, HO, HO, N, N, N]
    assert _texts("max_layers_16") == both
    # record and message bounds: R or D of 3 holds no message; from 4 on both hellos are found, with what is there
    b = _texts("bounds")
    assert b[:4] == [N, N, N, N] and b[4:8] == ["0,,,,", "0,,,,", "0,0,", "0,0,"]
    assert b[12:16] == b[36:40] == ["771,,,,", "771,,,,", "771,0,", "771,0,"]  # D = 6 and D = 41
    assert b[40] == CH_TEXT and b[42] == SH_TEXT
    assert b[41] == "771,4865-4866-49199-156-10,0-23-10-11,29-23-24,0-1-2"  # ten bytes short: the last two extensions
    # length1 >= 1 and five zero bytes: a hello at D = 15 (its ciphers lie past D), unknown from D = 16 on
    assert b[43:46] == ["771,,,,", N, "771,0,"] and b[46:52] == [N] * 6
    # ClientHello fields
    f = _texts("client_fields")
    assert f[0] == "771,,,," and f[1] == "771,,,,"                         # the session id swallows the rest
    # 200 entries are claimed: the ones that fit are used (the compression bytes 01 00 and what follows among them),
    # and E, from the count, lies past D
    assert f[2] == "771,1-2-3-4-256,,," and f[3].startswith("771,1-2-3-4-256-47-0-7-5-0-609-25088-") and f[3][-3:] == ",,,"
    # an odd length of 5: two entries, and E two bytes early: the list's length is read as 256, its first "extension"
    # is the real length field (47) with the real first type (0) as its length, the next is (7, 5 bytes)
    assert f[4] == "771,1-2,47-7-23-10-11-65281-43,29-23-24,0-1-2"
    assert f[5] == "771,1-2-3,0-23-10-11-65281-43,29-23-24,0-1-2"
    assert f[6] == f[7] == "771,4865-49199,0-23-10-11,29-23-24,0-1-2"       # cut by M, whatever D is
    assert f[8] == "771,4865-49199,0-23-10-11-65281,29-23-24,0-1-2" and f[9] == f[8]
    assert f[10] == f[8] and f[11] == "771,4865-49199,0-23-10-11-65281-43,29-23-24,0-1-2"
    assert f[12] == f[13] == "771,4865-49199,23,," and f[14] == "771,4865-49199,23-65281-35,,"
    assert f[15] == "771,4865-49199,23,,"
    assert f[16] == "771,4865-2586-6666-2827,10-11,29-23,0-1-2"  # 0xAAAA is GREASE, 0x0A1A is not
    assert f[17] == "771,,10,,"
    assert f[18] == "771,4865-49199,10-10-11-11,29-23,2"
    assert f[19:23] == ["771,4865-49199,10-10,,", "771,4865-49199,10-11,,0-1-2", "771,4865-49199,10-10-11,,0-1-2",
                        "771,4865-49199,10-11,,0-1-2"]
    assert f[23:27] == ["771,4865-49199,10-11,29-23-24,", "771,4865-49199,10-11-11,29-23-24,",
                        "771,4865-49199,10-11,29-23-24,", "771,4865-49199,10-11,29-23-24,255-100-9"]
    # the compression quirk moves E: without a method the length read is 0x2f00 and the first "extension" does not
    # fit; with two the list starts inside the length field
    assert f[27] == "771,4865-49199,,," and f[28] == "771,4865-49199,12032,,"
    assert f[29] == "771,,0-23-10-11-65281-43,29-23-24,0-1-2" and f[30] == "771,4865-49199,,,"
    assert f[31] == "769,65535-0-9-10-99-100-999-1000-9999-10000,,,"
    s = _texts("server_fields")
    assert s[:5] == ["771,4865,43-51", "772,4865,51-43", "772,4865,43", "771,4865,43", "771,4865,43"]
    assert s[5:9] == ["32540,4865,43-43", "771,4865,43-43", "772,2570,14906-43-64250", "770,4865,"]
    assert s[11] == "771,4865,23" and s[12] == SH_TEXT and s[13] == "772,4865,51-43"
    # the padding and block edges of MD5, and the longest text
    assert [len(t) for t in _texts("text_lengths")] == list(tc.TEXT_LENGTHS)
    long_case = BY_NAME["longest"]
    (text,) = _texts("longest")
    assert int(long_case.caplens[0]) == 65535 and len(text) > 190000 and len(text) <= 4 * 65535 + 16
    # records and flags
    fl = _texts("flags")
    assert fl[:20] == [CH_TEXT, CH_TEXT, HO, N, N, HO, N, HO, N, N, HO, N, HO, HO, HO, CH_TEXT, HO, N, N, CH_TEXT]
    pairs = fl[20:48]
    assert pairs[0::2] == [N] * 10 + [N, N, N, N] and pairs[1::2].count(CH_TEXT) >= 12
    assert fl[48] == N and fl[49] == CH_TEXT
    d = _texts("descriptors")
    assert [d[i] for i in (5, 11, 17, 21, 22, 30, 33, 36)] == [BD, BD, BD, N, BD, N, N, N]
    assert int(BY_NAME["descriptors"].offsets.max()) > 1 << 63  # the 64-bit wrap
    # batch shapes: hellos on both sides of every wave and block edge
    e = _texts("edges")
    assert [i for i, t in enumerate(e) if isinstance(t, str)] == list(tc.EDGES)
    assert all(isinstance(t, str) for t in _texts("all_hellos")) and BY_NAME["all_hellos"].n > tc.BLOCK
    assert set(_texts("no_hellos")) == {N} and BY_NAME["no_hellos"].n > tc.BLOCK
    m = _texts("n1025")
    assert [isinstance(m[i], str) for i in (63, 64, 65, 1023, 1024)] == [True, True, False, True, True]
    # capacities
    k, nb = tc.needs(BY_NAME["cap_exact"])
    exact = abi.tlsfp_totals_dict(tc.run_reference(BY_NAME["cap_exact"]).totals)
    assert (exact["client_n"] + exact["server_n"], exact["text_bytes"], exact["overflow"]) == (k, nb, 0)
    for name in ("cap_sizing", "cap_sizing_text", "cap_recs_short1", "cap_text_short1"):  # the full would-be values
        t = abi.tlsfp_totals_dict(tc.run_reference(BY_NAME[name]).totals)
        assert (t["client_n"] + t["server_n"], t["text_bytes"], t["candidates"], t["overflow"]) == (k, nb, k, 1)
    t = abi.tlsfp_totals_dict(tc.run_reference(BY_NAME["cap_hellos_short1"]).totals)
    assert (t["client_n"], t["server_n"], t["text_bytes"], t["candidates"], t["overflow"]) == (0, 0, 0, k, 1)
    no_text = tc.run_reference(BY_NAME["cap_no_text"])
    with_text = tc.run_reference(BY_NAME["cap_exact"])
    assert (no_text.records(k) == with_text.records(k)).all()  # digests and would-be positions without the text
    # the header's closed bound holds on every record of every case
    for c in CASES:
        if c.name in tc.OVERFLOWING or c.use_brief:
            continue
        got = tc.run_reference(c)
        for r in got.records(int(got.totals[abi.TLSFP_CANDIDATES])):
            assert int(r["text_len"]) <= 4 * int(c.caplens[int(r["index"])]) + 16, c.name


# ---------------------------------------------------------------- CPU: the reference's own vectors
def capture_case(b: PacketBatch, name: str, opts=None, **kw) -> tc.Case:
    """A capture through the parse's restatement: the records the device parse writes."""
    opts = opts or abi.make_opts()
    summary, layers, tuples = oracle.oracle_parse_tuples(b, opts)
    c = tc.Case(name, b.data, b.offsets, b.caplens, summary, np.ascontiguousarray(layers), ml=opts.max_layers,
                data_len=int(b.caplens.sum()), **kw)
    c.meta["tuples"] = tuples
    return c


_GOLDEN: dict = {}


def golden_batch() -> PacketBatch:
    if "b" not in _GOLDEN:
        _GOLDEN["b"] = read_pcap(VECTORS / "tls2_handshakes.pcap")  # tools/make_golden_tlsfp.py
    return _GOLDEN["b"]


def golden_rows(kind: str) -> list[tuple]:
    lines = (VECTORS / f"tls_fp_{kind}.txt").read_text().split("\n")
    assert tuple(lines[0].split("\t")) == tf.HEADER and lines[-1] == ""
    return [tuple(x.split("\t")) for x in lines[1:-1]]


def assert_rows(got: list[tuple], want: list[tuple], what: str) -> None:
    """Field by field; the two address columns as parsed addresses (IPv6 text has more than one spelling: the
    exemption of the reference's own test)."""
    assert len(got) == len(want), (what, len(got), len(want))
    for j, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 7
        for k in range(7):
            if k in (3, 5):
                assert ipaddress.ip_address(g[k]) == ipaddress.ip_address(w[k]), (what, j, k)
            else:
                assert g[k] == w[k], (what, j, k, g[k], w[k])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_reference_reproduces_the_golden_files(kind):
    client, server = KINDS[kind]
    c = capture_case(golden_batch(), f"tls2_{kind}", client=client, server=server)
    got = tc.run_reference(c)
    t = abi.tlsfp_totals_dict(got.totals)
    k = t["client_n"] + t["server_n"]
    assert k == ROWS[kind] and t["host_n"] == 0 and t["overflow"] == 0
    assert_rows(tf.rows(got.records(k), c.meta["tuples"], got.text), golden_rows(kind), kind)
    tc.assert_same(got, tc.model(c), c.name)
    longest = max(int(r["text_len"]) for r in got.records(k))
    assert not client or longest == 288  # the capture's longest fingerprint text
    if kind == "ch_sh":  # the example's tables of the most common fingerprints
        want = golden_rows(kind)
        for value, name in ((abi.TLSFP_CLIENT, "ClientHello"), (abi.TLSFP_SERVER, "ServerHello")):
            counts: dict = {}
            for w in want:
                if w[2] == name:
                    counts[w[0]] = counts.get(w[0], 0) + 1
            table = tf.top(got.records(k), value, None)
            assert dict(table) == counts and [n for _, n in table] == sorted(counts.values(), reverse=True)
            assert tf.top(got.records(k), value) == table[:10]


@pytest.mark.parametrize("name", CAPTURES)
def test_reference_equals_the_model_on_the_bundled_captures(name):
    matches = [p for p in FILES.iterdir() if p.name.endswith(f"__{name}.pcap")]
    assert len(matches) == 1
    b = read_pcap(matches[0])
    found = 0
    for kind in KINDS.values():
        c = capture_case(b, name, client=kind[0], server=kind[1])
        got = tc.run_reference(c)
        tc.assert_same(got, tc.model(c), name)
        found += int(got.totals[abi.TLSFP_CANDIDATES])
    assert found >= 2  # a hello under at least two of the three settings


def test_grease_and_zero_size_extension_captures():
    """What these two captures are there for: GREASE values leave the ClientHello's lists, and a zero-length
    extension is listed."""
    for name, check in (("tls_grease", lambda t: not any(int(v) in tf.GREASE for part in t.split(",")[1:4]
                                                          for v in part.split("-") if v)),
                        ("tls_zero_size_ext", lambda t: len(t.split(",")[2].split("-")) >= 2)):
        b = read_pcap(next(p for p in FILES.iterdir() if p.name.endswith(f"__{name}.pcap")))
        c = capture_case(b, name, server=False)
        got = tc.run_reference(c)
        recs = got.records(int(got.totals[abi.TLSFP_CLIENT_N]))
        assert len(recs) >= 1
        for r in recs:
            pos = int(r["text_pos"])
            assert check(bytes(got.text[pos:pos + int(r["text_len"])]).decode()), name


def test_md5_of_the_texts_the_contract_reaches():
    """Through the call itself: crafted ClientHellos whose text has every length from 7 to 130."""
    packets = [tc.pk(tc.hs(tc.ch_with_text_len(n)), n) for n in range(7, 131)]
    c = tc.make("md5", packets)
    got = tc.run_reference(c)
    recs = got.records(len(packets))
    assert [int(r["text_len"]) for r in recs] == list(range(7, 131))
    for r in recs:
        pos = int(r["text_pos"])
        assert bytes(r["md5"]) == hashlib.md5(bytes(got.text[pos:pos + int(r["text_len"])])).digest()


def _case_file(c: tc.Case, path: Path) -> None:
    want = tc.model(c)
    rec = tc.brief_of(c)[:c.n] if c.use_brief else c.summary
    head = np.array([c.n, c.dlen(), c.ml, 0 if c.use_brief else 1, int(c.client), int(c.server), c.max_hellos, c.maxr(),
                     c.cap(), int(c.want_text), int(c.want_disp), c.maxr() * 40, c.cap()], np.uint64)
    parts = [head, c.data[:c.dlen()], c.offsets, c.caplens, rec, c.layers, want.recs[:c.maxr() * 40]]
    parts += [want.text[:c.cap()]] if c.want_text else []
    parts += [want.disposition] if c.want_disp else []
    parts.append(want.totals)
    path.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))


def test_reference_under_sanitizers(tmp_path):
    """pcppx_tlsfp_reference and the library's MD5 in a stand-alone program (its own main, host compiler, no HIP,
    nothing loaded into python) built with ASan + UBSan: the case families in exact-size heap buffers, the results
    equal to the model's; MD5 against hashlib on texts of every length 0..130 (both sides of the 55 / 56 and 119 / 120
    padding edges and of the 64 and 128 block edges)."""
    gxx = shutil.which("g++")
    assert gxx is not None
    exe = tmp_path / "tlsfp_ref_check"
    csrc = abi.PKG_DIR / "csrc"
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), "-I", str(csrc),
                    str(abi.REPO_DIR / "tests" / "native" / "tlsfp_ref_check.cpp"),
                    str(csrc / "pcppx_tlsfp_ref.cpp"), "-o", str(exe)], check=True)
    files = []
    for name in ("bounds", "order", "client_fields", "server_fields", "text_lengths", "longest", "flags", "descriptors",
                 "max_layers_1", "edges", "n0", "n65_brief", "kinds_ch", "kinds_sh", "cap_exact", "cap_recs_short1",
                 "cap_text_short1", "cap_hellos_short1", "cap_no_text", "cap_sizing"):
        path = tmp_path / f"{name}.case"
        _case_file(BY_NAME[name], path)
        files.append(str(path))
    md5 = tmp_path / "lengths.md5"
    md5.write_bytes(b"".join(hashlib.md5(bytes((7 * i + 3) & 255 for i in range(n))).digest() for n in range(131)))
    files.append(str(md5))
    env = {"TMPDIR": str(tmp_path), "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(" ok\n") == len(files)


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_tlsfp_equals_reference(engine, case):
    want = tc.run_reference(case)
    got = tc.run_device(engine, case)
    tc.assert_same(got, want, case.name)
    if case.name in tc.OVERFLOWING:
        tc.assert_untouched(got, case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "n1025", "kinds_sh", "cap_text_short1", "cap_no_text"])
def test_gpu_tlsfp_is_repeatable_across_streams(engine, name):
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
def test_gpu_tlsfp_source_on_both_sides_of_4gib(engine):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32
    (the layout of test_frag.py's and test_tcpstream.py's cases): one hello lies across each line."""
    import torch

    import wide_cases as wc

    case = BY_NAME["n1025"]
    raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device="cuda:0")
    lay = wc.layout(raw.data_ptr(), 9)
    data = raw[lay.pad: lay.pad + lay.data_len]
    n, half = case.n, case.n // 2
    lens = case.caplens.astype(np.int64)
    offs = np.zeros(n, np.int64)
    for lo, hi, line in ((0, half, lay.lines[0]), (half, n, lay.lines[1])):
        run = np.cumsum(lens[lo:hi]) - lens[lo:hi]
        mid = (lo + hi) // 2 - lo
        while (lo + mid) % 3 == 2:  # a hello lies across the line
            mid += 1
        start = line - int(run[mid]) - int(lens[lo + mid]) // 2
        offs[lo:hi] = start + run
        k = lo + mid
        assert offs[k] < line < offs[k] + lens[k]
        src0 = int(case.offsets[lo])
        chunk = case.data[src0:src0 + int(lens[lo:hi].sum())]
        data[start:start + len(chunk)] = torch.from_numpy(chunk).to("cuda:0")
    order = np.random.default_rng(5).permutation(n)  # descriptors of both sides interleaved
    perm = lambda c, o: replace(c, offsets=o[order].astype(np.uint64), caplens=c.caplens[order],  # noqa: E731
                                summary=c.summary[order], layers=np.ascontiguousarray(c.layers[order]))
    wide, compact = perm(case, offs), perm(case, case.offsets)
    source = (data, torch.from_numpy(wide.offsets.view(np.int64)).to("cuda:0"),
              torch.from_numpy(wide.caplens.view(np.int32)).to("cuda:0"), lay.data_len)
    want = tc.run_reference(compact)
    assert int(want.totals[abi.TLSFP_CANDIDATES]) > 600
    assert {bool(o < wc.LINE) for o in wide.offsets} == {True, False}
    got = tc.run_device(engine, compact, source=source)
    tc.assert_same(got, want, "wide")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_gpu_golden_files_from_a_device_parse(engine, kind, tmp_path):
    """tls2 parsed on the device, fingerprinted on the device: the reference's output file, through the library and
    (ch_sh) through tools/tlsfp_file.py."""
    from pcapplusplus_amd.engine import tlsfp_on_device

    client, server = KINDS[kind]
    recs, text, tuples, disp, tot = tlsfp_on_device(engine, golden_batch(), client, server)
    assert tot["client_n"] + tot["server_n"] == ROWS[kind] == len(recs) and tot["host_n"] == 0
    assert_rows(tf.rows(recs, tuples, text), golden_rows(kind), kind)
    assert int((disp != 0).sum()) == ROWS[kind]
    if kind != "ch_sh":
        return
    out = tmp_path / "out.txt"
    run = subprocess.run([sys.executable, str(abi.REPO_DIR / "tools" / "tlsfp_file.py"), "-r",
                          str(VECTORS / "tls2_handshakes.pcap"), "-o", str(out), "-t", kind],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = out.read_text().split("\n")
    assert tuple(lines[0].split("\t")) == tf.HEADER
    assert_rows([tuple(x.split("\t")) for x in lines[1:-1]], golden_rows(kind), "tlsfp_file")
    assert "TLS ClientHello packets:              323" in run.stdout


@pytest.mark.gpu
def test_gpu_md5_words_steer_equal_fingerprints_together(engine):
    """Chained into an existing mover without leaving the device: the records' first MD5 words are pcppx_steer_device's
    key column (stride 40) over the batch of the fingerprint texts; equal fingerprints land in one bucket, and the
    buckets' counts are top()'s."""
    import torch

    c = BY_NAME["all_hellos"]
    run = tc.DeviceRun(c)
    st = torch.cuda.current_stream().cuda_stream
    run.launch(engine, st)
    k = tc.needs(c)[0]
    words = run.d_recs[:k * 40].view(torch.int64).reshape(k, 5)
    offsets = words[:, 2].contiguous()                       # text_pos
    caplens = (words[:, 3] & 0xFFFFFFFF).to(torch.int32)     # text_len
    buckets = 16
    spec = abi.make_steer_spec(key=abi.ptr(run.d_recs), key_stride=40, n_buckets=buckets)
    out_off = torch.empty(k, dtype=torch.int64, device="cuda:0")
    out_cap = torch.empty(k, dtype=torch.int32, device="cuda:0")
    out_idx = torch.empty(k, dtype=torch.int32, device="cuda:0")
    first = torch.empty(buckets + 1, dtype=torch.int32, device="cuda:0")
    pos = torch.empty(buckets + 1, dtype=torch.int64, device="cuda:0")
    totals = torch.empty(abi.STEER_TOTALS, dtype=torch.int64, device="cuda:0")
    engine.steer_device(run.d_text, offsets, caplens, k, tc.ETH, spec, out_off, out_cap, first, pos, totals, k,
                        out_index=out_idx, stream=st, data_len=tc.needs(c)[1])
    got = run.result()
    tot = abi.steer_totals_dict(totals.cpu().numpy().view(np.uint64))
    assert tot["steered_packets"] == k and tot["overflow"] == 0 and tot["bad_desc"] == 0
    recs = got.records(k)
    index, first = out_idx.cpu().numpy(), first.cpu().numpy()
    seen: dict = {}
    for b in range(buckets):
        members = index[first[b]:first[b + 1]]
        assert (np.diff(members) > 0).all()  # stable
        for j in members:
            h = bytes(recs["md5"][j])
            assert int.from_bytes(h[:4], "little") % buckets == b
            seen[h.hex()] = seen.get(h.hex(), 0) + 1
    table = tf.top(recs, abi.TLSFP_CLIENT, None) + tf.top(recs, abi.TLSFP_SERVER, None)
    # ch_k() of the odd packet numbers takes 20 of its 40 cipher values, sh_k() of the even ones its 7
    assert dict(table) == seen and len(seen) == 20 + 7 and sum(seen.values()) == k


# ---------------------------------------------------------------- the base scan's second step
N_WIDE, STEP = 66 * tc.BLOCK + 7, 64  # blocks a step of the base kernel takes
WIDE_TOTALS = {"client_n": 22531, "server_n": 22530, "text_bytes": 1441969, "candidates": 45061}  # frozen; none is zero


@functools.lru_cache(maxsize=None)
def wide():
    """(the 67-block case, what the reference leaves): built once, shared by the CPU and the GPU test."""
    case = tc.make("wide", tc.mixed(N_WIDE))
    return case, tc.run_reference(case)


def test_reference_past_64_blocks():
    case, want = wide()
    assert case.n == N_WIDE and (N_WIDE + tc.BLOCK - 1) // tc.BLOCK == STEP + 3
    tc.assert_same(want, tc.model(case), "wide")
    totals = abi.tlsfp_totals_dict(want.totals)
    assert totals["overflow"] == 0 and totals["host_n"] == 0 and totals["bad_desc"] == 0
    disp = want.disposition[:N_WIDE]
    for blk in (STEP, STEP + 1):  # the blocks behind the step line hold hellos of both kinds
        rows = disp[blk * tc.BLOCK:(blk + 1) * tc.BLOCK]
        assert len({int(d) for d in rows} - {tc.NONE, tc.HOST, tc.BAD}) == 2, blk
    assert all(v != 0 for v in WIDE_TOTALS.values()) and {k: totals[k] for k in WIDE_TOTALS} == WIDE_TOTALS


@pytest.mark.gpu
def test_gpu_tlsfp_past_64_blocks(engine):
    case, want = wide()
    tc.assert_same(tc.run_device(engine, case), want, "wide")
