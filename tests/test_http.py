"""pcppx_http_device: the first line and the header fields of the HTTP packets of a device batch (include/pcppx.h, http).

CPU: the ctypes mirrors match the header and every bad-argument family is refused before any device work;
pcppx_http_reference (the contract in plain C++ over host pointers) equals pcapplusplus_amd.http.model (the contract in
plain Python over bytes.find) on every case family of tests/http_cases.py, byte for byte, the 0xA5 fill of everything
else included (all of it but the totals on overflow); it reproduces what the real HttpRequestLayer / HttpResponseLayer
report on the reference's HTTP captures and on a crafted and mutated set (tests/golden/http/fields.npz, frozen by
tools/make_golden_http.py); analyze() gives HttpAnalyzer's tables; and the reference call runs clean under ASan + UBSan
in a stand-alone program.
GPU: pcppx_http_device equals pcppx_http_reference byte for byte on the same cases; two calls on two streams agree and
a repeat is bit-identical; HTTP packets on both sides of offset 2^32; the golden captures from a device parse.
"""
from __future__ import annotations

import ctypes as C
import json
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from collections import Counter
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import http_cases as hc
import oracle
from conftest import GOLDEN
from pcapplusplus_amd import abi
from pcapplusplus_amd import http as ht
from pcapplusplus_amd.pcap import PacketBatch, from_packets, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "http"
CASES = hc.cases()
BY_NAME = {c.name: c for c in CASES}
HTTP_PACKETS = {"4KHttpRequests.pcap": 385, "650HttpResponses.pcap": 682, "http-packets2.pcap": 115}


# ---------------------------------------------------------------- CPU: the ABI
def test_http_structs_match_header():
    fields = {"pcppx_http_spec": abi.HttpSpec, "pcppx_http_msg": abi.HttpMsg, "pcppx_http_field": abi.HttpField,
              "pcppx_http_out": abi.HttpOut}
    dtypes = {"pcppx_http_msg": abi.HTTP_MSG_DTYPE, "pcppx_http_field": abi.HTTP_FIELD_DTYPE}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = {"PCPPX_HTTP_NONE": abi.HTTP_NONE, "PCPPX_HTTP_MSG": abi.HTTP_MSG, "PCPPX_HTTP_HOST": abi.HTTP_HOST,
              "PCPPX_HTTP_BAD_DESC": abi.HTTP_BAD_DESC, "PCPPX_HTTP_REQUEST": abi.HTTP_REQUEST,
              "PCPPX_HTTP_RESPONSE": abi.HTTP_RESPONSE, "PCPPX_HTTP_KIND_REQUESTS": abi.HTTP_KIND_REQUESTS,
              "PCPPX_HTTP_KIND_RESPONSES": abi.HTTP_KIND_RESPONSES, "PCPPX_HTTP_FIELDS_NONE": abi.HTTP_FIELDS_NONE,
              "PCPPX_HTTP_FIELDS_WANTED": abi.HTTP_FIELDS_WANTED, "PCPPX_HTTP_FIELDS_ALL": abi.HTTP_FIELDS_ALL,
              "PCPPX_HTTP_TEXT_FIRST_LINE": abi.HTTP_TEXT_FIRST_LINE, "PCPPX_HTTP_TEXT_VALUES": abi.HTTP_TEXT_VALUES,
              "PCPPX_HTTP_METHOD_UNKNOWN": abi.HTTP_METHOD_UNKNOWN, "PCPPX_HTTP_VERSION_UNKNOWN": abi.HTTP_VERSION_UNKNOWN,
              "PCPPX_HTTP_FIRST_LINE_COMPLETE": abi.HTTP_FIRST_LINE_COMPLETE,
              "PCPPX_HTTP_HEADER_COMPLETE": abi.HTTP_HEADER_COMPLETE,
              "PCPPX_HTTP_HAS_CONTENT_LENGTH": abi.HTTP_HAS_CONTENT_LENGTH,
              "PCPPX_HTTP_CONTENT_LENGTH_RANGE": abi.HTTP_CONTENT_LENGTH_RANGE, "PCPPX_HTTP_HAS_VALUE": abi.HTTP_HAS_VALUE,
              "PCPPX_HTTP_FIRST": abi.HTTP_FIRST, "PCPPX_HTTP_NO_NAME": abi.HTTP_NO_NAME,
              "PCPPX_HTTP_MAX_NAMES": abi.HTTP_MAX_NAMES, "PCPPX_HTTP_NAME_MAX": abi.HTTP_NAME_MAX,
              "PCPPX_HTTP_MSGS": abi.HTTP_MSGS, "PCPPX_HTTP_REQUESTS": abi.HTTP_REQUESTS,
              "PCPPX_HTTP_RESPONSES": abi.HTTP_RESPONSES, "PCPPX_HTTP_FIELDS": abi.HTTP_FIELDS,
              "PCPPX_HTTP_TEXT_BYTES": abi.HTTP_TEXT_BYTES, "PCPPX_HTTP_HOST_N": abi.HTTP_HOST_N,
              "PCPPX_HTTP_BAD_DESC_N": abi.HTTP_BAD_DESC_N, "PCPPX_HTTP_HEADER_BYTES": abi.HTTP_HEADER_BYTES,
              "PCPPX_HTTP_FIELDS_LINKED": abi.HTTP_FIELDS_LINKED, "PCPPX_HTTP_OVERFLOW": abi.HTTP_OVERFLOW,
              "PCPPX_HTTP_TOTALS": abi.HTTP_TOTALS, "PCPPX_ABI_VERSION": abi.ABI_VERSION}
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu\\n", sizeof(pcppx_http_spec), sizeof(pcppx_http_msg), sizeof(pcppx_http_field), '
           'sizeof(pcppx_http_out));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    # the spec is 4 + 4 * 1 + 8 + 8 * 32 = 272 bytes
    assert [int(x) for x in out[0].split()] == [C.sizeof(cls) for cls in fields.values()] == [272, 48, 24, 56]
    assert [int(x) for x in out[1].split()] == list(consts.values())
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        if t in dtypes:  # the numpy mirror too
            dt, at = dtypes[t].fields[f][:2]
            assert (at, dt.itemsize) == (int(off), int(size)), name
        seen += 1
    assert seen == sum(len(cls._fields_) for cls in fields.values())
    assert abi.ABI_VERSION == 7 and len(abi.HTTP_TOTAL_NAMES) == abi.HTTP_TOTALS


def test_http_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_http_device", "pcppx_http_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_http_spec(hc.NAMES)
    o = abi.HttpOut(1, 1, 1, 1, 1, 1, 1, 1)
    return dict(b=b, r=r, ml=6, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _names(a, names):
    a["s"] = abi.make_http_spec(names)


def _name_len(a, k, v):
    a["s"].name_len[k] = v


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_msgs": lambda a: _set(a, "o", "msgs", None),
    "null_fields": lambda a: _set(a, "o", "fields", None),
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
    "kinds_0": lambda a: _set(a, "s", "kinds", 0),
    "kinds_4": lambda a: _set(a, "s", "kinds", 4),
    "kinds_255": lambda a: _set(a, "s", "kinds", 255),
    "fields_3": lambda a: _set(a, "s", "fields", 3),
    "fields_255": lambda a: _set(a, "s", "fields", 255),
    "text_4": lambda a: _set(a, "s", "text", 4),
    "text_255": lambda a: _set(a, "s", "text", 255),
    "n_names_9": lambda a: _set(a, "s", "n_names", 9),
    "n_names_255": lambda a: _set(a, "s", "n_names", 255),
    "name_len_0": lambda a: _name_len(a, 1, 0),
    "name_len_33": lambda a: _name_len(a, 1, 33),
    "name_len_beyond_n_names": lambda a: _name_len(a, 4, 1),
    "name_len_last_beyond": lambda a: _name_len(a, 7, 32),
    "upper_case_first": lambda a: _names(a, ("Host",)),
    "upper_case_last": lambda a: _names(a, ("host", "content-typE")),
    "upper_case_a": lambda a: _names(a, ("hAst",)),
    "upper_case_z": lambda a: _names(a, ("hoZt",)),
    "equal_names": lambda a: _names(a, ("host", "accept", "host")),
    "equal_names_adjacent": lambda a: _names(a, ("a", "a")),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_http_device's, pcppx_http_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_http_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_http_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_http_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_http_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # names that differ only in length or by a byte, '@' and '[' (the neighbours of 'A' and 'Z'), a brief instead of the
    # summary, absent optional outputs and an empty batch pass
    for names in (("host", "host "), ("a@[", "a@\\"), tuple("abcdefgh"), ("x" * 32,)):
        c = replace(BY_NAME["headers"], names=names)
        assert int(hc.run_reference(c).totals[abi.HTTP_OVERFLOW]) == 0
    for name in ("n65_brief", "cap_no_text_no_disp", "n0", "spec_no_names", "spec_8_names"):
        assert int(hc.run_reference(BY_NAME[name]).totals[abi.HTTP_OVERFLOW]) == 0
    empty = hc.run_reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.HTTP_TOTALS
    hc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_the_model(case):
    got = hc.run_reference(case)
    hc.assert_same(got, hc.model(case), case.name)
    if case.name in hc.OVERFLOWING:
        assert int(got.totals[abi.HTTP_OVERFLOW]) == 1
        hc.assert_untouched(got, case.name)
    else:
        assert int(got.totals[abi.HTTP_OVERFLOW]) == 0


def _msgs(name: str, **kw) -> np.ndarray:
    return hc.run_reference(replace(BY_NAME[name], **kw)).messages()


def _disp(name: str) -> list:
    c = BY_NAME[name]
    return [int(d) for d in hc.run_reference(c).disposition[:c.n]]


def _uri(c: hc.Case, m) -> bytes:
    at = int(c.offsets[int(m["index"])]) + int(m["layer_offset"]) + int(m["a_offset"])
    return c.data[at:at + int(m["a_len"])].tobytes()


def test_cases_cover_the_contract():
    """The block size the cases are built around is the kernels', and the families reach the paths they name: the
    values here are worked out by hand from the rules of include/pcppx.h."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kHttpBlockPk\s*=\s*(\d+)", txt).group(1)) == hc.BLOCK
    assert max(c.n for c in CASES) <= 2100
    FLC, HC, HCL, RNG = (abi.HTTP_FIRST_LINE_COMPLETE, abi.HTTP_HEADER_COMPLETE, abi.HTTP_HAS_CONTENT_LENGTH,
                         abi.HTTP_CONTENT_LENGTH_RANGE)
    U, V = abi.HTTP_METHOD_UNKNOWN, abi.HTTP_VERSION_UNKNOWN
    lines = BY_NAME["lines"]
    m = hc.run_reference(lines).messages()
    assert len(m) == lines.n
    rq = {name: m[k] for k, (name, _) in enumerate(hc.REQUEST_LINES)}
    at = len(hc.REQUEST_LINES)
    meth = m[at:at + 9]
    rs = {name: m[at + 9 + k] for k, (name, _) in enumerate(hc.RESPONSE_LINES)}
    L = lambda x: int(x["layer_len"])  # noqa: E731
    line = lambda x: (int(x["method"]), int(x["version"]), int(x["first_line_len"]), int(x["flags"]) & FLC)  # noqa: E731
    # rule 4
    assert line(rq["get"]) == (0, 2, 26, FLC) and _uri(lines, rq["get"]) == b"/index.html"
    assert [int(x) for x in meth["method"]] == list(range(9)) and all(int(x) & FLC for x in meth["flags"])
    for name in ("L_below_4", "L_4_no_space", "space_at_0", "no_space", "unknown_method",
                 "lower_case_method", "method_of_8_bytes"):
        assert line(rq[name]) == (U, V, L(rq[name]), 0) and int(rq[name]["a_len"]) == 0, name
    for name in ("no_version", "version_cut_v_plus_8"):
        assert line(rq[name]) == (0, V, L(rq[name]), 0) and int(rq[name]["a_offset"]) == 0, name
    assert line(rq["space_at_last_byte"]) == (6, V, 8, 0)  # the method is known with its space at L - 1
    assert line(rq["version_at_v_plus_9"]) == (0, 2, 14, 0) and _uri(lines, rq["version_at_v_plus_9"]) == b"/"
    assert line(rq["version_unknown_text"]) == (0, V, 16, FLC) and line(rq["version_no_dot"]) == (0, V, 16, FLC)
    assert line(rq["version_0_9"])[:2] == (0, 0) and line(rq["version_1_0"])[:2] == (2, 1)
    assert line(rq["no_newline"]) == (0, 2, L(rq["no_newline"]), 0)
    assert (int(rq["empty_uri"]["a_offset"]), int(rq["empty_uri"]["a_len"])) == (4, 0)
    assert _uri(lines, rq["uri_with_spaces"]) == b"/a b c" and _uri(lines, rq["two_versions"]) == b"/x"
    assert int(rq["two_versions"]["version"]) == 1
    assert _uri(lines, rq["space_http_in_header"]) == b"/x\r\nX: y" and int(rq["space_http_in_header"]["n_fields"]) == 0
    assert line(rq["lf_only"]) == (0, 2, 15, FLC) and int(rq["lf_only"]["flags"]) & HC
    assert _uri(lines, rq["almost_version"]) == b"/ HTTP" and int(rq["almost_version"]["version"]) == V  # the first " HTTP/"
    # rule 5
    st = lambda x: (int(x["version"]), int(x["status_code"]), int(x["a_len"]), int(x["first_line_len"]))  # noqa: E731
    assert st(rs["ok"]) == (2, 200, 2, 17) and _uri(lines, rs["ok"]) == b"OK" and int(rs["ok"]["method"]) == U
    assert st(rs["L_below_8"]) == (V, 0, 0, 7) and st(rs["L_8"]) == (2, 0, 0, 8)
    assert st(rs["not_http"])[:2] == (V, 0) and st(rs["version_unknown"])[:2] == (V, 0)
    assert st(rs["version_1_0"])[:3] == (1, 404, 9) and st(rs["version_0_9"])[:2] == (0, 200)
    for name in ("L_11", "L_12", "L_13", "L_14_lf", "no_newline", "code_not_digits", "code_space", "empty_message_crlf",
                 "empty_message_lf"):
        assert st(rs[name])[:3] == (2, 0, 0), name
    assert st(rs["message_cr_only"])[:3] == (2, 200, 1) and _uri(lines, rs["message_lf"]) == b"Moved Permanently"
    assert st(rs["newline_before_13"]) == (2, 200, 11, 13) and _uri(lines, rs["newline_before_13"]) == b"OK and more"
    assert st(rs["code_599"])[1] == 599 and st(rs["code_099"])[1] == 99
    assert _uri(lines, rs["no_space_before_message"]) == b"K"
    # rules 6-8: the request of each header case, every field
    hd = replace(BY_NAME["headers"], fields=abi.HTTP_FIELDS_ALL)
    got = hc.run_reference(hd)
    hm, hf = got.messages(), got.records()
    by = {name: (hm[2 * k], hf[int(hm[2 * k]["first_field"]):][:int(hm[2 * k]["n_rec"])])
          for k, (name, _) in enumerate(hc.FIELD_CASES)}
    hdr = lambda name: (int(by[name][0]["header_len"]) - 26, int(by[name][0]["n_fields"]),  # noqa: E731
                        bool(int(by[name][0]["flags"]) & HC))
    fld = lambda name: [(int(f["name_offset"]) - 26, int(f["name_len"]), int(f["value_offset"]) - 26 if int(f["flags"]) & 1  # noqa: E731
                         else None, int(f["value_len"])) for f in by[name][1]]
    assert hdr("plain") == (len(hc.FIELD_CASES[0][1]), 3, True)
    assert fld("plain") == [(0, 4, 6, 11), (19, 10, 31, 5), (38, 6, 46, 3)]
    assert hdr("first_line_len_is_L") == (0, 0, True) and hdr("end_at_once_crlf") == (2, 0, True)
    assert hdr("end_at_once_lf") == (1, 0, True) and hdr("end_at_once_cr") == (4, 0, True)
    assert hdr("lf_lf") == (6, 1, True) and hdr("crlf_crlf") == (8, 1, True)
    assert fld("line_starts_with_colon")[0] == (0, 0, 2, 5) and hdr("line_starts_with_colon") == (20, 2, True)
    assert fld("colon_only_line_last") == [(0, 4, 6, 1), (9, 0, None, 0)] and hdr("colon_only_line_last") == (10, 2, True)
    assert fld("colon_behind_nul") == [(0, 5, 7, 16)] and hdr("colon_behind_nul") == (2, 1, False)
    assert hdr("nul_then_more") == (17, 2, True) and fld("nul_then_more")[1] == (6, 4, 12, 1)
    assert hdr("nul_at_field_start") == (6, 1, False)
    assert fld("name_colon_at_last_byte")[1] == (9, 4, None, 0) and fld("spaces_to_the_end")[1] == (9, 4, None, 0)
    assert fld("spaces_then_newline")[0] == (0, 4, 8, 0) and fld("value_empty_crlf") == [(0, 4, 5, 0), (7, 4, 12, 0)]
    assert fld("no_colon_line")[0] == (0, 15, None, 0) and fld("colon_on_a_later_line")[0] == (0, 20, None, 0)
    assert fld("colon_at_e") == [(0, 4, None, 0), (4, 0, 5, 3)] and hdr("colon_at_e") == (10, 2, True)
    assert fld("no_newline_with_value") == [(0, 4, 6, 11)] and fld("no_newline_no_colon") == [(0, 7, None, 0)]
    assert fld("value_cr_inside") == [(0, 1, 3, 3)] and fld("value_ends_cr_cr") == [(0, 1, 3, 2)]
    assert fld("many_spaces") == [(0, 1, 8, 3)] and fld("tab_is_value") == [(0, 1, 2, 2)]
    assert hdr("header_incomplete") == (24, 2, False) and hdr("header_incomplete_cut") == (17, 2, False)
    assert hdr("empty_name_last") == (12, 2, True)
    assert hdr("linear")[1] == 702
    ids = lambda name: [(int(f["name_id"]), int(f["flags"]) >> 1) for f in by[name][1]]  # noqa: E731
    assert ids("repeated_host") == [(0, 1), (0, 0), (0, 0), (255, 0)]
    assert ids("name_trailing_space") == [(255, 0), (0, 1)] and ids("upper_lower") == [(0, 1), (1, 1), (2, 1)]
    assert ids("name_non_ascii") == [(255, 0), (255, 0)] and ids("body_behind") == [(0, 1)]
    ln = hc.run_reference(BY_NAME["long_names"])
    k = 2 * [n for n, _ in hc.FIELD_CASES].index("name_32_bytes")
    f32 = ln.records()[int(ln.messages()[k]["first_field"]):][:2]
    assert [int(x) for x in f32["name_id"]] == [2, 255]
    k = 2 * [n for n, _ in hc.FIELD_CASES].index("name_trailing_space")
    assert [int(x) for x in ln.records()[int(ln.messages()[k]["first_field"]):][:2]["name_id"]] == [0, 1]
    # rule 9
    cm = hc.run_reference(BY_NAME["content_length"]).messages()
    want = [0, 12, -5, 2147483647, 0, 0, 0, 42, 7, 0, 0, 0, 12, 12, 0, 0, 9, 0]
    rng = [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0]
    for k in range(len(hc.CONTENT_LENGTHS)):
        for x in (cm[2 * k], cm[2 * k + 1]):
            assert int(x["content_length"]) == want[k] and (int(x["flags"]) & (HCL | RNG)) == HCL | (RNG * rng[k]), k
    tail = cm[2 * len(hc.CONTENT_LENGTHS):]
    assert [(int(x["content_length"]), int(x["flags"]) & HCL) for x in tail] == [(0, HCL), (0, HCL), (77, HCL), (0, 0), (0, 0)]
    # every disposition, flag, method, version and kind is reached; text of both sorts
    allm = np.concatenate([hc.run_reference(c).messages() for c in CASES if c.name not in hc.OVERFLOWING])
    # (an incomplete first line reaches the layer's end, so its header is an end-of-header field: 0 cannot happen)
    assert {int(x) for x in allm["flags"]} >= {1, 2, 3, 5, 7, 15} and set(range(10)) == {int(x) for x in allm["method"]}
    assert {int(x) for x in allm["version"]} == {0, 1, 2, 3} and {int(x) for x in allm["kind"]} == {0, 1}
    allf = np.concatenate([hc.run_reference(c).records() for c in CASES if c.name not in hc.OVERFLOWING])
    assert {int(x) for x in allf["flags"]} == {0, 1, 2, 3}
    seen = set()
    for c in CASES:
        if c.want_disp and c.name not in hc.OVERFLOWING:
            seen |= set(_disp(c.name))
    assert seen == {hc.NONE, hc.MSG, hc.HOST, hc.BAD}
    # rule 3 over all flag combinations, and a recorded layer wins over any flag
    fl = _disp("flags")
    for k, f in enumerate(hc.flag_combinations()):
        assert fl[k] == (hc.HOST if ht.needs_host(f, 3, hc.ML) else hc.NONE), hex(f)
    assert fl[:256].count(hc.NONE) == 10 and fl[256:] == [hc.MSG, hc.MSG]
    r = _disp("records")
    M, N, H = hc.MSG, hc.NONE, hc.HOST
    assert r == [M, N, N, N, N, M, M, M, M, M, N, M, N, M, H, N, M, M, M]
    rm = _msgs("records")
    assert [int(x) for x in rm["layer_len"][1:4]] == [3, 0, 0] and [int(x) for x in rm["header_len"][1:4]] == [3, 0, 0]
    assert int(rm["kind"][4]) == 1 and int(rm["version"][4]) == V and int(rm["status_code"][4]) == 0
    assert int(rm[-2]["method"]) == U and int(rm[-2]["n_fields"]) == 0 and int(rm[-1]["status_code"]) == 0
    assert int(rm[-1]["n_fields"]) == 1
    assert set(_disp("max_layers_1")) == {H} and set(_disp("max_layers_4")) == {M}
    d = _disp("descriptors")
    assert [d[i] for i in (5, 11, 17, 22, 30)] == [hc.BAD] * 4 + [N]
    assert int(BY_NAME["descriptors"].offsets.max()) > 1 << 63  # the 64-bit wrap
    # the parse's own records find every message, the crafted ones too
    pm = abi.http_totals_dict(hc.run_reference(BY_NAME["parsed_mixed"]).totals)
    assert pm["msgs"] >= 200 and pm["host_n"] == 0
    assert abi.http_totals_dict(hc.run_reference(BY_NAME["parsed_ml3"]).totals)["host_n"] == 64
    # batch shapes
    for n in hc.SIZES:
        for share in hc.SHARES:
            t = abi.http_totals_dict(hc.run_reference(BY_NAME[f"n{n}_s{share}"]).totals)
            assert t["msgs"] == ({1: len(range(0, n, 97)), 100: n}[share] + (1 if share == 1 and n >= 128 else 0))
    # kinds choose the messages; fields and text choose the records and the bytes, never the messages' own values
    full = hc.run_reference(BY_NAME["spec_k3_f2_t3"])
    fm = full.messages()
    for kinds in (1, 2, 3):
        for fields in (0, 1, 2):
            for text in (0, 1, 2, 3):
                got = hc.run_reference(BY_NAME[f"spec_k{kinds}_f{fields}_t{text}"])
                gm = got.messages()
                keep = fm[[bool((kinds >> int(x)) & 1) for x in fm["kind"]]]
                for f in ("index", "content_length", "header_len", "first_line_len", "n_fields", "a_offset", "a_len",
                          "status_code", "kind", "method", "version", "flags"):
                    assert (gm[f] == keep[f]).all(), (kinds, fields, text, f)
                gf = got.records()
                assert (fields == 0) == (len(gf) == 0)
                if fields == 1:
                    assert (gf["name_id"] != 255).all()
                want_text = (int(gm["a_len"].sum()) if text & 1 else 0) + \
                    (int(gf["value_len"][gf["name_id"] != 255].sum()) if text & 2 else 0)
                assert int(got.totals[abi.HTTP_TEXT_BYTES]) == want_text == int(gm["text_len"].sum())
    assert len(hc.run_reference(BY_NAME["spec_no_names"]).records()) == 0  # WANTED without a name wants nothing
    # capacities: the totals hold the full would-be values under every overflow
    m_, k_, nb = hc.needs(BY_NAME["cap_exact"])
    for name in ("cap_exact", "cap_spec_exact", "cap_no_text", "cap_roomy") + hc.OVERFLOWING:
        t = abi.http_totals_dict(hc.run_reference(BY_NAME[name]).totals)
        assert (t["msgs"], t["fields"], t["text_bytes"], t["overflow"]) == (m_, k_, nb, int(name in hc.OVERFLOWING)), name
    no_text, with_text = hc.run_reference(BY_NAME["cap_no_text"]), hc.run_reference(BY_NAME["cap_exact"])
    assert (no_text.records(k_) == with_text.records(k_)).all()  # positions and lengths without the text
    assert (no_text.messages(m_) == with_text.messages(m_)).all()


# ---------------------------------------------------------------- CPU: the reference's own vectors
def read_pcapng(path: Path) -> PacketBatch:
    """The enhanced packet blocks of a little-endian pcapng file with one interface."""
    raw, pos, out = path.read_bytes(), 0, []
    while pos + 12 <= len(raw):
        kind, size = struct.unpack("<II", raw[pos:pos + 8])
        if kind == 6:
            cap = struct.unpack("<I", raw[pos + 20:pos + 24])[0]
            out.append(raw[pos + 28:pos + 28 + cap])
        pos += size
    return from_packets(out)


def capture_case(b: PacketBatch, name: str, opts=None, **kw) -> hc.Case:
    """A capture through the parse's restatement: the records the device parse writes."""
    opts = opts or abi.make_opts()
    summary, layers = oracle.oracle_parse(b, opts)
    return hc.Case(name, np.concatenate([b.data, np.zeros(1, np.uint8)]), b.offsets, b.caplens, summary,
                   np.ascontiguousarray(layers).reshape(b.n, opts.max_layers), ml=opts.max_layers,
                   data_len=int(b.caplens.sum()), **kw)


_GOLDEN: dict = {}
GOLDEN_FILES = sorted(str(f) for f in np.load(VECTORS / "fields.npz", allow_pickle=False)["files"])
ALL_FIELDS = dict(names=hc.NAMES, fields=abi.HTTP_FIELDS_ALL, text=3)


def frozen() -> dict:
    if "frozen" not in _GOLDEN:
        _GOLDEN["frozen"] = hc.load_frozen(VECTORS / "fields.npz")  # tools/make_golden_http.py
    return _GOLDEN["frozen"]


def golden_batch(name: str) -> PacketBatch:
    if name not in _GOLDEN:
        path = VECTORS / name
        _GOLDEN[name] = read_pcapng(path) if name.endswith(".pcapng") else read_pcap(path)
    return _GOLDEN[name]


def golden_case(name: str) -> hc.Case:
    if ("case", name) not in _GOLDEN:
        _GOLDEN[("case", name)] = capture_case(golden_batch(name), name, **ALL_FIELDS)
    return _GOLDEN[("case", name)]


def frozen_rows(b: PacketBatch, msgs, fields, text) -> dict:
    """A call's records (every field, names NAMES, text 3) in the shape of fields.npz's entries, per source packet with
    a message; the end-of-header field, which has no record, is left out, and a content length out of an int's range
    is None."""
    text = bytes(text)
    per = {}
    for m in msgs:
        i, lo = int(m["index"]), int(m["layer_offset"])
        d = b.packet(i)[lo:lo + int(m["layer_len"])]
        pos, fl = int(m["text_pos"]), int(m["flags"])
        assert text[pos:pos + int(m["a_len"])] == d[int(m["a_offset"]):int(m["a_offset"]) + int(m["a_len"])]
        rec = fields[int(m["first_field"]):int(m["first_field"]) + int(m["n_rec"])]
        assert len(rec) == int(m["n_fields"])
        rows = []
        for k, f in enumerate(rec):
            no, vo = int(f["name_offset"]), int(f["value_offset"])
            nxt = int(rec[k + 1]["name_offset"]) if k + 1 < len(rec) else None
            name = d[no:no + int(f["name_len"])]
            first = None
            if int(f["name_id"]) != abi.HTTP_NO_NAME:
                assert ht._lower(name).decode("latin-1") == hc.NAMES[int(f["name_id"])]
                first = (int(f["flags"]) >> 1) & 1
                tp = int(f["text_pos"])
                assert text[tp:tp + int(f["text_len"])] == d[vo:vo + int(f["value_len"])]
            rows.append([name.hex(), d[vo:vo + int(f["value_len"])].hex(), None if nxt is None else nxt - no, first])
        per[i] = [int(m["kind"]), int(m["header_len"]), int(m["n_fields"]), (fl >> 1) & 1, int(m["first_line_len"]),
                  int(m["method"]), int(m["version"]), d[int(m["a_offset"]):int(m["a_offset"]) + int(m["a_len"])].hex(),
                  int(m["status_code"]), fl & 1, None if fl & abi.HTTP_CONTENT_LENGTH_RANGE else int(m["content_length"]),
                  (fl >> 2) & 1, rows]
    return per


def assert_frozen(per: dict, name: str) -> None:
    """Exactly the packets the real reference builds an HTTP layer in, and what it reports of each."""
    want = frozen()[name]
    assert len(want) == golden_batch(name).n
    for i, w in enumerate(want):
        g = per.get(i)
        assert (g is None) == (w is None), (name, i)
        if w is None:
            continue
        assert g[:10] == w[:10] and g[11] == w[11], (name, i, g[:12], w[:12])
        assert g[10] is None or g[10] == w[10], (name, i)
        wf = [f for f in w[12] if not f[3]]
        end = [f for f in w[12] if f[3]]
        assert len(wf) == len(g[12]) and len(end) <= 1, (name, i)
        for k, (gf, f) in enumerate(zip(g[12], wf)):
            size = gf[2] if gf[2] is not None else g[1] - (end[0][2] if end else 0) - \
                (g[4] + sum(x[2] for x in wf[:k]))
            assert gf[:2] == f[:2] and size == f[2], (name, i, k, gf, f)
            lowered = ht._lower(bytes.fromhex(f[0])).decode("latin-1")
            assert gf[3] == (f[4] if lowered in hc.NAMES else None), (name, i, k)


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_reference_reproduces_the_real_http_layers(name):
    """No packet is left out: a packet has a message exactly where the reference builds an HTTP layer, and HOST and NONE
    packets are exactly those where it builds none; header_len is the parse's hdr_len."""
    c = golden_case(name)
    got = hc.run_reference(c)
    t = abi.http_totals_dict(got.totals)
    assert t["host_n"] == 0 and t["overflow"] == 0 and t["bad_desc"] == 0
    msgs = got.messages()
    assert_frozen(frozen_rows(golden_batch(name), msgs, got.records(), got.text[:t["text_bytes"]]), name)
    if name in HTTP_PACKETS:
        assert t["msgs"] == HTTP_PACKETS[name]
    for m in msgs:
        lay = c.layers[int(m["index"])]
        e = [x for x in lay[:int(c.summary["n_layers"][int(m["index"])])] if int(x["proto"]) in (6, 7)][0]
        assert int(e["hdr_len"]) == int(m["header_len"]) and int(e["data_len"]) == int(m["layer_len"])
    hc.assert_same(got, hc.model(c), name)


def test_golden_data_holds_the_oddities():
    """What the crafted set is there for, read off the real layers' frozen answers."""
    crafted = [p for p in frozen()["crafted.pcap"] if p is not None]
    assert len(frozen()["crafted.pcap"]) >= 1500 and len(crafted) >= 1200
    assert sum(1 for p in crafted if not p[9]) >= 50 and sum(1 for p in crafted if not p[3]) >= 300
    assert sum(1 for p in crafted if p[2] == 0) >= 50                                  # messages without a field
    assert sum(1 for p in crafted for f in p[12] if not f[3] and f[1] == "") >= 300    # fields without a value
    assert sum(1 for p in crafted for f in p[12] if not f[3] and not f[4]) >= 30       # repeated names
    # (the reference builds a request layer only behind a known method)
    assert {p[5] for p in crafted if p[0] == 0} == set(range(9)) and {p[6] for p in crafted} == {0, 1, 2, 3}
    assert any(p[3] and not any(f[3] for f in p[12]) for p in crafted)  # complete by an empty name, not by an end field


def _tables_from_frozen(name: str) -> dict:
    out = {"requests": 0, "responses": 0, "request_header_bytes": 0, "response_header_bytes": 0, "methods": Counter(),
           "hosts": Counter(), "status": Counter(), "content_types": Counter(), "with_content_length": 0,
           "content_length_sum": 0}
    esc = lambda h: bytes.fromhex(h).decode("latin-1").encode("unicode_escape").decode("ascii")  # noqa: E731
    for p in frozen()[name]:
        if p is None:
            continue
        by_name = {}
        for f in p[12]:
            if not f[3] and f[4]:
                by_name[bytes.fromhex(f[0]).lower()] = f[1]
        if p[0] == 0:
            out["requests"] += 1
            out["request_header_bytes"] += p[1]
            out["methods"][abi.HTTP_METHODS[p[5]] if p[5] < 9 else "unknown"] += 1
            if b"host" in by_name:
                out["hosts"][esc(by_name[b"host"])] += 1
            continue
        out["responses"] += 1
        out["response_header_bytes"] += p[1]
        if p[11]:
            out["with_content_length"] += 1
            out["content_length_sum"] += p[10]
        if b"content-type" in by_name:
            out["content_types"][esc(by_name[b"content-type"]).split(";")[0]] += 1
        out["status"][f"{p[8]} {esc(p[7])}"] += 1
    return {k: dict(v) if isinstance(v, Counter) else v for k, v in out.items()}


@pytest.mark.parametrize("name", ["4KHttpRequests.pcap", "650HttpResponses.pcap"])
def test_analyze_gives_http_analyzers_tables(name):
    c = replace(golden_case(name), fields=abi.HTTP_FIELDS_WANTED)
    got = hc.run_reference(c)
    t = abi.http_totals_dict(got.totals)
    tables = ht.analyze(got.messages(), got.records(), got.text[:t["text_bytes"]], hc.NAMES)
    assert tables == _tables_from_frozen(name)
    assert tables["requests"] + tables["responses"] == HTTP_PACKETS[name]
    assert tables["request_header_bytes"] + tables["response_header_bytes"] == t["header_bytes"]
    assert len(tables["hosts"]) + len(tables["status"]) > 3


def _case_file(c: hc.Case, path: Path) -> None:
    want = hc.model(c)
    rec = hc.brief_of(c)[:c.n] if c.use_brief else c.summary
    spec = np.frombuffer(bytes(hc.spec_of(c)), np.uint8)
    head = np.array([c.n, c.dlen(), c.ml, 0 if c.use_brief else 1, c.maxm(), c.maxf(), c.cap(), int(c.want_text),
                     int(c.want_disp)], np.uint64)
    parts = [head, spec, c.data[:c.dlen()], c.offsets, c.caplens, rec, c.layers, want.msgs[:c.maxm() * 48],
             want.fields[:c.maxf() * 24]]
    parts += [want.text[:c.cap()]] if c.want_text else []
    parts += [want.disposition[:c.n]] if c.want_disp else []
    parts.append(want.totals)
    path.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))


def test_reference_under_sanitizers(tmp_path):
    """pcppx_http_reference in a stand-alone program (its own main, host compiler, no HIP, nothing loaded into python)
    built with ASan + UBSan: the case families in exact-size heap buffers, the results equal to the model's."""
    gxx = shutil.which("g++")
    assert gxx is not None
    exe = tmp_path / "http_ref_check"
    csrc = abi.PKG_DIR / "csrc"
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), "-I", str(csrc),
                    str(abi.REPO_DIR / "tests" / "native" / "http_ref_check.cpp"),
                    str(csrc / "pcppx_http_ref.cpp"), "-o", str(exe)], check=True)
    files = []
    for name in ("lines", "headers", "content_length", "fuzz", "fuzz_all", "long_names", "flags", "records",
                 "max_layers_1", "descriptors", "parsed_mixed", "n65_s100", "n1025_s1", "n0", "n65_brief",
                 "spec_k1_f2_t3", "spec_k2_f1_t2", "spec_k3_f0_t1", "spec_no_names", "cap_exact", "cap_msgs_short1",
                 "cap_fields_short1", "cap_text_short1", "cap_spec_short1", "cap_no_text", "cap_sizing"):
        path = tmp_path / f"{name}.case"
        _case_file(BY_NAME[name], path)
        files.append(str(path))
    env = {"TMPDIR": str(tmp_path), "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(" ok\n") == len(files)


TOOL = [sys.executable, str(abi.REPO_DIR / "tools" / "http_file.py")]


def assert_tool_tables(stdout: str, name: str) -> None:
    assert json.loads(stdout) == _tables_from_frozen(name)


def test_http_file_tool_without_gpu(tmp_path):
    """tools/http_file.py --reference: HttpAnalyzer's tables and the rows of a golden capture, without a GPU."""
    name = "650HttpResponses.pcap"
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "--analyze"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert_tool_tables(run.stdout, name)
    out = tmp_path / "rows.txt"
    run = subprocess.run(TOOL + ["-r", str(VECTORS / "TwoHttpRequests.pcap"), "--reference", "-o", str(out)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    c = replace(golden_case("TwoHttpRequests.pcap"), fields=abi.HTTP_FIELDS_WANTED)
    assert out.read_text().split("\n") == [ht.format_row(r) for r in hc.run_reference(c).rows()] + [""]
    assert out.read_text().count("\n") >= 4


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_http_equals_reference(engine, case):
    want = hc.run_reference(case)
    got = hc.run_device(engine, case)
    hc.assert_same(got, want, case.name)
    if case.name in hc.OVERFLOWING:
        hc.assert_untouched(got, case.name)


@pytest.mark.gpu
def test_gpu_http_sizing_then_exact(engine):
    """The sizing call (no room at all) gives the three sizes; the call with exactly that room succeeds."""
    base = BY_NAME["cap_exact"]
    t = abi.http_totals_dict(hc.run_device(engine, BY_NAME["cap_sizing"]).totals)
    assert t["overflow"] == 1
    exact = replace(base, out_msgs=t["msgs"], out_fields=t["fields"], text_cap=t["text_bytes"])
    got = hc.run_device(engine, exact)
    assert int(got.totals[abi.HTTP_OVERFLOW]) == 0
    hc.assert_same(got, hc.run_reference(exact), "exact")
    no_text = hc.run_device(engine, BY_NAME["cap_no_text"])
    assert (no_text.records(t["fields"]) == got.records(t["fields"])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1025_s100", "n2049_s1", "spec_k2_f2_t3", "cap_text_short1", "cap_no_text"])
def test_gpu_http_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = hc.run_reference(case)
    runs = [hc.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        hc.assert_same(r.result(), want, f"{name} run {k}")


@pytest.mark.gpu
def test_gpu_http_source_on_both_sides_of_4gib(engine):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32
    (the layout of test_dns.py's case): one HTTP message lies across each line."""
    import torch

    import wide_cases as wc

    case = BY_NAME["n1025_s100"]
    raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device="cuda:0")
    lay = wc.layout(raw.data_ptr(), 9)
    data = raw[lay.pad: lay.pad + lay.data_len]
    n, half = case.n, case.n // 2
    lens = case.caplens.astype(np.int64)
    offs = np.zeros(n, np.int64)
    for lo, hi, line in ((0, half, lay.lines[0]), (half, n, lay.lines[1])):
        run = np.cumsum(lens[lo:hi]) - lens[lo:hi]
        mid = (lo + hi) // 2 - lo
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
    want = hc.run_reference(compact)
    assert int(want.totals[abi.HTTP_MSGS]) == n
    assert {bool(o < wc.LINE) for o in wide.offsets} == {True, False}
    got = hc.run_device(engine, compact, source=source)
    hc.assert_same(got, want, "wide")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_gpu_golden_captures_from_a_device_parse(engine, name):
    """Parsed on the device, walked on the device: what the real HTTP layers report; for the responses' capture also
    HttpAnalyzer's tables through tools/http_file.py."""
    from pcapplusplus_amd.engine import http_on_device

    b = golden_batch(name)
    spec = abi.make_http_spec(hc.NAMES, abi.HTTP_FIELDS_ALL, 3)
    msgs, fields, text, disp, tot = http_on_device(engine, b, spec)
    assert tot["host_n"] == 0 and tot["msgs"] == len(msgs) == int((disp == abi.HTTP_MSG).sum())
    assert_frozen(frozen_rows(b, msgs, fields, text), name)
    if name in HTTP_PACKETS:
        assert tot["msgs"] == HTTP_PACKETS[name]
    if name != "650HttpResponses.pcap":
        return
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--analyze"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert_tool_tables(run.stdout, name)
