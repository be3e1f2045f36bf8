"""pcppx_sip_device: the SIP messages, their header fields and their SDP bodies of a device batch (include/pcppx.h, sip).

CPU: the ctypes mirrors match the header and every bad-argument family is refused before any device work;
pcppx_sip_reference (the contract in plain C++ over host pointers) equals pcapplusplus_amd.sip.model (the contract in
plain Python) on every case family of tests/sip_cases.py, byte for byte, the 0xA5 fill of everything else included (all
of it but the totals on overflow); the cases reach every rule and flag; the reference call reproduces what the real
SipRequestLayer / SipResponseLayer / SdpLayer report on the reference's SIP captures and on a crafted and mutated set
(tests/golden/sip/expected.npz, frozen by tools/make_golden_sip.py); calls() gives the per-call table; and the reference
call runs clean under ASan + UBSan in a stand-alone program.
GPU: pcppx_sip_device equals pcppx_sip_reference byte for byte on the same cases; two calls on two streams agree and a
repeat is bit-identical; SIP packets on both sides of offset 2^32; the golden captures from a device parse.
"""
from __future__ import annotations

import ctypes as C
import json
import re
import shutil
import subprocess
import sys
import tempfile
from collections import Counter
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import oracle
import sip_cases as sc
from conftest import GOLDEN
from pcapplusplus_amd import abi
from pcapplusplus_amd import sip as sp
from pcapplusplus_amd.pcap import PacketBatch, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "sip"
CASES = sc.cases()
BY_NAME = {c.name: c for c in CASES}
GOLDEN_FILES = ("crafted.pcap", "many_protocols_sip.pcap", "packet_examples.pcap")
REAL_FILES = GOLDEN_FILES[1:]


# ---------------------------------------------------------------- CPU: the ABI
def test_sip_structs_match_header():
    fields = {"pcppx_sip_spec": abi.SipSpec, "pcppx_sip_msg": abi.SipMsg, "pcppx_sip_field": abi.SipField,
              "pcppx_sip_sdp": abi.SipSdp, "pcppx_sip_out": abi.SipOut}
    dtypes = {"pcppx_sip_msg": abi.SIP_MSG_DTYPE, "pcppx_sip_field": abi.SIP_FIELD_DTYPE,
              "pcppx_sip_sdp": abi.SIP_SDP_DTYPE}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = {"PCPPX_SIP_NONE": abi.SIP_NONE, "PCPPX_SIP_MSG": abi.SIP_MSG, "PCPPX_SIP_HOST": abi.SIP_HOST,
              "PCPPX_SIP_BAD_DESC": abi.SIP_BAD_DESC, "PCPPX_SIP_REQUEST": abi.SIP_REQUEST,
              "PCPPX_SIP_RESPONSE": abi.SIP_RESPONSE, "PCPPX_SIP_METHOD_UNKNOWN": abi.SIP_METHOD_UNKNOWN,
              "PCPPX_SIP_VIA_PORT": abi.SIP_VIA_PORT, "PCPPX_SIP_VIA_HEURISTIC": abi.SIP_VIA_HEURISTIC,
              "PCPPX_SIP_FIRST_LINE_COMPLETE": abi.SIP_FIRST_LINE_COMPLETE,
              "PCPPX_SIP_HEADER_COMPLETE": abi.SIP_HEADER_COMPLETE,
              "PCPPX_SIP_HAS_CONTENT_LENGTH": abi.SIP_HAS_CONTENT_LENGTH,
              "PCPPX_SIP_CONTENT_LENGTH_RANGE": abi.SIP_CONTENT_LENGTH_RANGE,
              "PCPPX_SIP_VERSION_KNOWN": abi.SIP_VERSION_KNOWN, "PCPPX_SIP_HAS_SDP": abi.SIP_HAS_SDP,
              "PCPPX_SIP_CARRIER_TCP": abi.SIP_CARRIER_TCP, "PCPPX_SIP_SDP_HAS_OWNER": abi.SIP_SDP_HAS_OWNER,
              "PCPPX_SIP_SDP_HAS_AUDIO": abi.SIP_SDP_HAS_AUDIO, "PCPPX_SIP_SDP_HAS_VIDEO": abi.SIP_SDP_HAS_VIDEO,
              "PCPPX_SIP_MSGS": abi.SIP_MSGS, "PCPPX_SIP_REQUESTS": abi.SIP_REQUESTS,
              "PCPPX_SIP_RESPONSES": abi.SIP_RESPONSES, "PCPPX_SIP_FIELDS": abi.SIP_FIELDS,
              "PCPPX_SIP_TEXT_BYTES": abi.SIP_TEXT_BYTES, "PCPPX_SIP_HOST_N": abi.SIP_HOST_N,
              "PCPPX_SIP_BAD_DESC_N": abi.SIP_BAD_DESC_N, "PCPPX_SIP_HEADER_BYTES": abi.SIP_HEADER_BYTES,
              "PCPPX_SIP_FIELDS_LINKED": abi.SIP_FIELDS_LINKED, "PCPPX_SIP_SDPS": abi.SIP_SDPS,
              "PCPPX_SIP_BY_HEURISTIC": abi.SIP_BY_HEURISTIC, "PCPPX_SIP_OVERFLOW": abi.SIP_OVERFLOW,
              "PCPPX_SIP_TOTALS": abi.SIP_TOTALS, "PCPPX_ABI_VERSION": abi.ABI_VERSION}
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu %zu\\n", sizeof(pcppx_sip_spec), sizeof(pcppx_sip_msg), sizeof(pcppx_sip_field), '
           'sizeof(pcppx_sip_sdp), sizeof(pcppx_sip_out));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(cls) for cls in fields.values()] == [272, 48, 24, 32, 72]
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
    assert abi.ABI_VERSION == 7 and len(abi.SIP_TOTAL_NAMES) == abi.SIP_TOTALS and len(abi.SIP_METHODS) == 14


def test_sip_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_sip_device", "pcppx_sip_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_sip_spec(sc.NAMES)
    o = abi.SipOut(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _names(a, names):
    a["s"] = abi.make_sip_spec(names)


def _name_len(a, k, v):
    a["s"].name_len[k] = v


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_msgs": lambda a: _set(a, "o", "msgs", None),
    "null_fields": lambda a: _set(a, "o", "fields", None),
    "null_sdps": lambda a: _set(a, "o", "sdps", None),
    "reserved_set": lambda a: _set(a, "o", "reserved", 1),
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
    "upper_case_first": lambda a: _names(a, ("Call-id",)),
    "upper_case_last": lambda a: _names(a, ("call-id", "froM")),
    "equal_names": lambda a: _names(a, ("call-id", "to", "call-id")),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_sip_device's, pcppx_sip_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_sip_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_sip_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_sip_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_sip_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # a brief instead of the summary, absent optional outputs and an empty batch pass
    for name in ("n65_brief", "cap_no_text_no_disp", "n0_all", "spec_no_names", "spec_8_names"):
        assert int(sc.run_reference(BY_NAME[name]).totals[abi.SIP_OVERFLOW]) == 0
    empty = sc.run_reference(BY_NAME["n0_all"])
    assert list(empty.totals) == [0] * abi.SIP_TOTALS
    sc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_the_model(case):
    got = sc.run_reference(case)
    sc.assert_same(got, sc.model(case), case.name)
    if case.name in sc.OVERFLOWING:
        assert int(got.totals[abi.SIP_OVERFLOW]) == 1
        sc.assert_untouched(got, case.name)
    else:
        assert int(got.totals[abi.SIP_OVERFLOW]) == 0


def _disp(name: str) -> list:
    c = BY_NAME[name]
    return [int(d) for d in sc.run_reference(c).disposition[:c.n]]


def _by_packet(name: str, **kw):
    """(the case, its dispositions, its messages by source packet, its SDP records by source packet)."""
    c = replace(BY_NAME[name], **kw)
    got = sc.run_reference(c)
    return (c, [int(d) for d in got.disposition[:c.n]], {int(m["index"]): m for m in got.messages()},
            {int(s["index"]): s for s in got.bodies()})


def _a(c: sc.Case, m) -> bytes:
    at = int(c.offsets[int(m["index"])]) + int(m["layer_offset"]) + int(m["a_offset"])
    return c.data[at:at + int(m["a_len"])].tobytes()


def test_cases_cover_the_contract():
    """The block size the cases are built around is the kernels', and the families reach the rules and flags they name:
    the values here are worked out by hand from the rules of include/pcppx.h."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kSipBlockPk\s*=\s*(\d+)", txt).group(1)) == sc.BLOCK
    assert max(c.n for c in CASES) <= 2100
    M, N, H, B = sc.MSG, sc.NONE, sc.HOST, sc.BAD
    FLC, HC, HCL, RNG, VK, SDP, TCP = (abi.SIP_FIRST_LINE_COMPLETE, abi.SIP_HEADER_COMPLETE,
                                       abi.SIP_HAS_CONTENT_LENGTH, abi.SIP_CONTENT_LENGTH_RANGE, abi.SIP_VERSION_KNOWN,
                                       abi.SIP_HAS_SDP, abi.SIP_CARRIER_TCP)
    c, d, m, _ = _by_packet("lines")
    order = sc.METHOD_LINES + sc.NEAR_MISSES + sc.REQUEST_LINES + sc.CODE_LINES + sc.REJECTED + sc.RESPONSE_LINES
    at = {name: 3 * k for k, (name, _) in enumerate(order)}  # UDP port path, TCP port path, heuristic path
    trio = lambda name: d[at[name]:at[name] + 3]  # noqa: E731
    # rules 7 and 8: each of the 14 methods on the three paths, and the near misses of each on none
    for k, meth in enumerate(abi.SIP_METHODS):
        assert trio(f"method_{meth}") == [M, M, M]
        x = [m[at[f"method_{meth}"] + j] for j in range(3)]
        assert [int(y["method"]) for y in x] == [k] * 3 and [int(y["via"]) for y in x] == [0, 0, 1]
        assert [int(y["flags"]) & TCP for y in x] == [0, TCP, 0] and all(int(y["flags"]) & VK for y in x)
        assert _a(c, x[0]) == f"sip:u{k}@example.com".encode()
        for kind in ("lower", "no_space", "space_at_0", "longer", "shorter"):
            assert trio(f"{kind}_{meth}") == [N, N, N], (kind, meth)
    assert trio("L_3") == [N, N, N] and trio("L_4_no_space") == [N, N, N]
    assert trio("L_4_space_last") == [M, M, N]  # the method is known with its space at L - 1; no second space
    # rule 9: no " SIP/" (or a cut one): no URI, no version, the line's end searched from the byte before the layer
    for name in ("no_version", "no_second_space", "cut_v_plus_5", "cut_v_plus_6", "cut_inside_sip"):
        assert trio(name) == [M, M, N], name
        x = m[at[name]]
        assert int(x["flags"]) & VK == 0 and int(x["a_len"]) == 0 and int(x["a_offset"]) == 0, name
    assert int(m[at["no_version"]]["first_line_len"]) == 28 and int(m[at["no_version"]]["flags"]) & FLC
    assert int(m[at["cut_v_plus_6"]]["first_line_len"]) == 18 and int(m[at["cut_v_plus_6"]]["flags"]) & FLC == 0
    for name, ok in (("cut_v_plus_7", N), ("cut_v_plus_8", M)):  # known from v + 7 on; the heuristic wants 7 bytes more
        assert trio(name) == [M, M, ok], name
        assert int(m[at[name]]["flags"]) & VK and _a(c, m[at[name]]) == b"sip:b"
    assert trio("empty_uri") == [M, M, N] and int(m[at["empty_uri"]]["flags"]) & VK
    assert (int(m[at["empty_uri"]]["a_offset"]), int(m[at["empty_uri"]]["a_len"])) == (0, 0)
    assert trio("uri_with_spaces") == [M, M, N] and _a(c, m[at["uri_with_spaces"]]) == b"sip:a b c"
    assert trio("two_versions") == [M, M, M] and _a(c, m[at["two_versions"]]) == b"sip:a"
    assert _a(c, m[at["version_in_header"]]) == b"sip:a\r\nX: y" and int(m[at["version_in_header"]]["n_fields"]) == 1
    assert trio("version_in_header") == [M, M, N]
    assert trio("lf_only") == [M, M, M] and int(m[at["lf_only"]]["first_line_len"]) == 22
    for name in ("short_version", "version_6_bytes", "http_version", "no_second_space", "key_but_unknown_method"):
        assert trio(name)[2] == N, name  # the heuristic's four checks, and a key without a method
    assert trio("short_version")[:2] == [M, M] and int(m[at["short_version"]]["flags"]) & VK  # "SIP/2" is a version
    assert trio("almost_sip") == [M, M, N] and _a(c, m[at["almost_sip"]]) == b"sip:b SIP"
    assert trio("key_but_unknown_method") == [N, N, N]
    # the byte in front of the layer: 0x0A gives first_line_len 0, and the request line is the first field
    base = 3 * len(order)
    names4 = ("no_version", "no_version_no_newline", "cut_v_plus_6", "cut_inside_sip")
    for li, last in enumerate(sc.LAST_BYTES):
        for ni, name in enumerate(names4):
            for way in range(2):
                x = m[base + 2 * (li * 4 + ni) + way]
                if last == 0x0A:
                    assert int(x["first_line_len"]) == 0 and int(x["flags"]) & FLC and int(x["n_fields"]) >= 1
                else:
                    assert int(x["first_line_len"]) == int(m[at[name]]["first_line_len"]) > 0
    # rules 7 and 10: every accepted status code, and the rejected ones
    for code in sorted(sp.CODES):
        assert trio(f"code_{code}") == [M, M, M]
        assert {int(m[at[f"code_{code}"] + j]["status_code"]) for j in range(3)} == {sp.AS_INT.get(code, code)}
        assert _a(c, m[at[f"code_{code}"]]) == b"Text" and int(m[at[f"code_{code}"]]["method"]) == 14
    assert all(trio(name) == [N, N, N] for name, _ in sc.REJECTED)
    for name in ("L_11", "no_space_at_11", "not_digits", "letters", "high_bytes", "no_space_at_all"):
        assert trio(name) == [N, N, N], name
    for name, code in (("wraps_to_100", 100), ("wraps_to_200_high", 200)):  # the 16-bit sum wraps onto an accepted code
        assert trio(name) == [M, M, M], name
        assert int(m[at[name]]["status_code"]) == code
    assert int(m[at["wraps_to_100"]]["a_len"]) == 0  # the line ends inside the code: no status text
    assert trio("L_12") == [M, M, M] and int(m[at["L_12"]]["a_len"]) == 0  # s + 4 = 11 = L - 1
    assert trio("L_13") == [M, M, M] and int(m[at["L_13"]]["a_len"]) == 0 and int(m[at["L_13"]]["flags"]) & FLC == 0
    assert _a(c, m[at["ok"]]) == b"OK" and _a(c, m[at["no_newline"]]) == b"Ringing and o"  # the last byte is dropped
    assert _a(c, m[at["no_newline_cr_before_end"]]) == b"Ringing" and _a(c, m[at["resp_lf_only"]]) == b"Not Found"
    assert trio("not_sip") == [N, M, N]  # TCP has no version test; the layer then has no status
    x = m[at["not_sip"] + 1]
    assert int(x["status_code"]) == 0 and int(x["flags"]) & VK == 0 and int(x["a_len"]) == 0
    assert trio("long_version") == [N, N, M] and int(m[at["long_version"] + 2]["status_code"]) == 0
    assert trio("s_plus_4_at_L_minus_1") == [N, N, M]
    assert trio("s_plus_4_at_L") == [N, N, H] and trio("s_plus_4_at_L_plus_1") == [N, N, H]  # undefined: the host's
    assert trio("s_plus_4_far") == [N, N, H]
    assert trio("heuristic_bad_code") == [N, N, N] and trio("heuristic_no_space_behind_code") == [N, N, N]
    assert trio("version_6") == [N, N, M]  # "SIP/2. 200 OK": the space at 6, the code at 7 on the heuristic path alone
    # rules 5 and 6
    pc, pd, pm, _ = _by_packet("ports")
    np_, nq = len(sc.PORT_PAYLOADS), len(sc.PORTS)
    row = lambda name: pd[np_ * [n for n, _, _ in sc.PORTS].index(name):][:np_]  # noqa: E731
    for name in ("dhcp_68_67", "dhcp_67_68", "dhcp_67_67", "vxlan_dst", "dhcp_and_sip", "sip_and_vxlan"):
        assert row(name) == [N] * np_, name
    for name in ("sip_src", "sips_dst"):
        assert row(name) == [M, M, M, N, N, N], name  # "SIP/2.0 200" has 11 bytes
    for name in ("not_dhcp_68_68", "vxlan_src", "plain", "dns_dst", "dns_src"):
        assert row(name) == [M, M, M, N, N, N], name  # the heuristic path: "SIP/2.0 200" is below 12 bytes
    for p in sorted(sp.GATED_EITHER):
        assert row(f"gated_dst_{p}") == row(f"gated_src_{p}") == [H, H, H, H, N, N], p
    for p in sorted(sp.GATED_DST):
        assert row(f"gated_dst_{p}") == [H, H, H, H, N, N] and row(f"gated_src_{p}") == [M, M, M, N, N, N], p
    tcp_rows = pd[np_ * nq:np_ * nq + 2 * nq]
    for k, (name, s, dport) in enumerate(sc.PORTS):  # TCP: the SIP ports alone
        assert tcp_rows[2 * k:2 * k + 2] == ([M, M] if {s, dport} & {5060, 5061} else [N, N]), name
    half = len(pd) // 2  # the same packets under the parse's own flags: DNS and the tunnels are named by the parse
    own = lambda name: pd[half + np_ * [n for n, _, _ in sc.PORTS].index(name):][:np_]  # noqa: E731
    assert own("dns_dst") == [N, N, N, N, N, N] and own("vxlan_dst") == [H] * np_ and own("gated_dst_2152") == [H] * np_
    assert own("plain") == [M, M, M, N, N, N] and own("sip_src") == row("sip_src")
    # rules 2 and 3 over all flag combinations
    fl = _disp("flags")
    for k, f in enumerate(sc.flag_combinations()):
        host = f & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW) or \
            (f & abi.F_NEEDS_HOST_L7 and not f & abi.F_L7_KNOWN)
        none = not f & abi.F_NEEDS_HOST_L7 or f & (abi.F_L7_HTTP | abi.F_L7_SSL | abi.F_L7_DNS)
        assert fl[k] == (H if host else N if none else M), hex(f)
    assert fl.count(M) == 1
    # rule 4
    assert _disp("records") == [M, M, N, N, N, N, N, N, N, N, N, N, M, N, M, M, M, N, N, N, H, N, M, N]
    _, _, rm, _ = _by_packet("records")
    assert int(rm[1]["layer_len"]) == int(rm[0]["layer_len"]) - 4  # the trailer's bytes are not the message's
    assert int(rm[12]["layer_len"]) == 30 and int(rm[15]["flags"]) & TCP and int(rm[22]["flags"]) & TCP
    assert _disp("cut_by_caplen") == [M, N, N, N, N, M]
    assert set(_disp("max_layers_1")) == {H} and set(_disp("max_layers_2")) == {H} and set(_disp("max_layers_3")) == {M}
    dd = _disp("descriptors")
    assert [dd[i] for i in (5, 11, 17, 22, 30)] == [B] * 4 + [N]
    assert int(BY_NAME["descriptors"].offsets.max()) > 1 << 63  # the 64-bit wrap
    # rules 12 and 13, the header side
    cc, cd, cm, cs = _by_packet("content")
    ck = {name: k for k, (name, _) in enumerate(sc.CONTENT_CASES)}
    cl = lambda name: (int(cm[ck[name]]["content_length"]), int(cm[ck[name]]["flags"]) & (HCL | RNG | SDP))  # noqa: E731
    n_sdp = len(sc.SDP)
    assert cl("plain") == (n_sdp, HCL | SDP) and cl("length_first") == (n_sdp, HCL | SDP)
    assert cl("compact_l") == (0, 0) and cl("negative") == (-5, HCL) and cl("zero") == (0, HCL)
    assert cl("above_2_31") == (0, HCL | RNG) and cl("huge") == (0, HCL | RNG) and cl("absent") == (0, 0)
    assert cl("at_2_31_minus_1") == (2147483647, HCL | SDP) and cl("no_value") == (0, HCL)
    assert cl("two_lengths") == (0, HCL) and cl("length_upper") == (7, HCL | SDP)
    assert cl("type_lower_name")[1] & SDP and not cl("type_upper_value")[1] & SDP
    assert cl("type_in_the_middle")[1] & SDP and not cl("type_cut")[1] & SDP
    assert cl("type_behind_nul")[1] & SDP and not cl("type_nul_inside")[1] & SDP  # find() over all the value's bytes
    assert not cl("two_types_first_wins")[1] & SDP and cl("two_types_first_sdp")[1] & SDP
    assert not cl("type_compact_c")[1] & SDP and not cl("type_no_value")[1] & SDP and not cl("no_type")[1] & SDP
    assert not cl("no_body")[1] & SDP and not cl("header_incomplete")[1] & SDP  # L == header_len
    assert cl("response_with_sdp")[1] & SDP and int(cm[ck["response_with_sdp"]]["status_code"]) == 183
    assert cl("length_behind_nul") == (12, HCL | SDP)  # atoi stops at the NUL
    assert int(cm[ck["header_incomplete"]]["flags"]) & HC == 0 and int(cm[ck["plain"]]["flags"]) & HC
    x = cm[len(sc.CONTENT_CASES) + len(sc.SDP_CASES)]  # 0x0A in front: the request line is field 0
    assert int(x["first_line_len"]) == 0 and int(x["n_fields"]) == 3 and int(x["flags"]) & SDP
    assert int(cm[ck["first_line_len_0"]]["first_line_len"]) == 28 and int(cm[ck["first_line_len_0"]]["n_fields"]) == 2
    want = cs[ck["plain"]]
    assert bytes(want["owner_ipv4"]) == bytes([192, 168, 1, 20]) and int(want["flags"]) == 7
    assert (int(want["audio_port"]), int(want["video_port"]), int(want["n_fields"])) == (49170, 51372, 8)
    assert int(want["offset"]) == int(cm[ck["plain"]]["header_len"]) and int(want["len"]) == n_sdp
    # the NUL in a wanted value: the field's value runs to the line's end
    got = sc.run_reference(BY_NAME["content"])
    vm = got.messages()[ck["value_behind_nul"]]
    vf = got.records()[int(vm["first_field"]):][:int(vm["n_rec"])]
    assert [(int(f["name_id"]), int(f["value_len"])) for f in vf] == [(0, 12), (1, 1)]
    # rule 13, the body side
    sk = {name: len(sc.CONTENT_CASES) + k for k, (name, _) in enumerate(sc.SDP_CASES)}
    body = lambda name: (bytes(cs[sk[name]]["owner_ipv4"]), int(cs[sk[name]]["audio_port"]),  # noqa: E731
                         int(cs[sk[name]]["video_port"]), int(cs[sk[name]]["flags"]))
    ip = lambda t: bytes(int(x) for x in t.split("."))  # noqa: E731
    Z = bytes(4)
    assert body("lf_only") == (ip("10.1.2.3"), 4000, 4002, 7) and body("no_o") == (Z, 4000, 0, 2)
    assert body("five_tokens") == (Z, 4000, 0, 2) and body("seven_tokens")[0] == ip("1.2.3.4")
    assert body("ip6") == (Z, 0, 6000, 4) and body("not_in")[3] == 0 and body("in_with_nul")[3] == 0
    assert body("tabs") == (ip("1.2.3.4"), 4000, 0, 3) and body("two_o_first_wins")[0] == ip("1.2.3.4")
    assert body("two_o_first_bad")[3] == 0 and body("upper_o") == (ip("9.8.7.6"), 1234, 0, 3)
    assert body("o_no_value") == (Z, 5, 0, 2) and body("o_no_separator_at_end")[3] == 0 and body("o_space_name")[3] == 0
    assert body("space_not_skipped") == (ip("1.2.3.4"), 7, 0, 3)  # tokens are split on white space anyway
    for name in ("addr_leading_zero", "addr_double_zero", "addr_three", "addr_five", "addr_trailing_dot",
                 "addr_leading_dot", "addr_double_dot", "addr_256", "addr_4_digits", "addr_hex", "addr_all_zero",
                 "addr_nul_head", "addr_letters"):
        assert body(name)[3] & 1 == 0 and body(name)[0] == Z, name
    assert body("addr_zero_octet")[0] == ip("10.0.0.1") and body("addr_255")[0] == ip("255.255.255.255")
    assert body("addr_nul_tail")[0] == ip("1.2.3.4") and body("addr_no_newline")[0] == ip("7.7.7.7")
    assert body("several_m") == (Z, 4000, 6000, 6) and body("m_one_token")[3] == 0 and body("m_audio_upper")[3] == 0
    assert body("m_audio_nul") == (Z, 4, 0, 2)  # "audio\0" is another token; atoi stops at the NUL
    assert body("port_65535")[1:3] == (65535, 0) and body("port_70000")[1:3] == (70000 - 65536, 65535)
    assert body("port_huge")[1:3] == (65535, 0) and body("port_long_max")[1:3] == (65535, 65535)
    assert body("port_long_min")[1:3] == (0, 0) and body("port_plus")[1:3] == (80, 0) and body("port_text")[1:3] == (40, 0)
    assert body("port_zero") == (Z, 0, 0, 2) and body("no_line_end")[1] == 4000
    assert int(cs[sk["empty_line_ends_it"]]["n_fields"]) == 1 and body("empty_line_ends_it")[3] == 0
    assert int(cs[sk["starts_with_newline"]]["n_fields"]) == 0 and int(cs[sk["nul_at_start"]]["n_fields"]) == 8
    assert body("nul_ends_it") == (Z, 4000, 0, 2) and int(cs[sk["no_separator_lines"]]["n_fields"]) == 3
    assert body("no_separator_lines")[1] == 9 and body("separator_on_a_later_line")[3] == 1
    assert int(cs[sk["one_byte"]]["n_fields"]) == 1 and int(cs[sk["one_byte"]]["len"]) == 1
    # every disposition, flag, method, kind and path is reached; field flags of every sort
    alive = [c for c in CASES if c.name not in sc.OVERFLOWING]
    allm = np.concatenate([sc.run_reference(c).messages() for c in alive])
    bits = 0
    for f in {int(x) for x in allm["flags"]}:
        bits |= f
    assert bits == 127 and {int(x) for x in allm["method"]} == set(range(15))
    assert {int(x) for x in allm["kind"]} == {0, 1} and {int(x) for x in allm["via"]} == {0, 1}
    alls = np.concatenate([sc.run_reference(c).bodies() for c in alive])
    assert {int(x) for x in alls["flags"]} == set(range(8))
    allf = np.concatenate([sc.run_reference(c).records() for c in alive])
    assert {int(x) for x in allf["flags"]} == {0, 1, 2, 3}
    seen = set()
    for c in alive:
        if c.want_disp:
            seen |= set(_disp(c.name))
    assert seen == {N, M, H, B}
    # the parse's own records find the messages
    pm = abi.sip_totals_dict(sc.run_reference(BY_NAME["parsed_mixed"]).totals)
    assert pm["msgs"] >= 200 and pm["by_heuristic"] >= 30 and pm["sdps"] >= 60
    assert abi.sip_totals_dict(sc.run_reference(BY_NAME["parsed_ml2"]).totals)["host_n"] == 64
    # batch shapes
    for n in sc.SIZES:
        t = {share: abi.sip_totals_dict(sc.run_reference(BY_NAME[f"n{n}_{share}"]).totals) for share in sc.SHARES}
        assert t["last"]["msgs"] == (1 if n else 0) and t["1in100"]["msgs"] <= len(range(0, n, 100))
        assert t["all"]["msgs"] + t["all"]["host_n"] + t["all"]["bad_desc"] <= n and t["all"]["msgs"] >= n * 3 // 4
        if n:
            assert _disp(f"n{n}_last")[-1] == M
    # kinds choose the messages; fields and text choose the records and the bytes, never the messages' own values
    full = sc.run_reference(BY_NAME["spec_k3_f2_t3"])
    fm = full.messages()
    for kinds in (1, 2, 3):
        for fields in (0, 1, 2):
            for text in (0, 1, 2, 3):
                got = sc.run_reference(BY_NAME[f"spec_k{kinds}_f{fields}_t{text}"])
                gm = got.messages()
                keep = fm[[bool((kinds >> int(x)) & 1) for x in fm["kind"]]]
                for f in ("index", "content_length", "header_len", "first_line_len", "n_fields", "a_offset", "a_len",
                          "status_code", "kind", "method", "via", "flags"):
                    assert (gm[f] == keep[f]).all(), (kinds, fields, text, f)
                gf = got.records()
                assert (fields == 0) == (len(gf) == 0)
                if fields == 1:
                    assert (gf["name_id"] != 255).all()
                want_text = (int(gm["a_len"].sum()) if text & 1 else 0) + \
                    (int(gf["value_len"][gf["name_id"] != 255].sum()) if text & 2 else 0)
                assert int(got.totals[abi.SIP_TEXT_BYTES]) == want_text == int(gm["text_len"].sum())
                assert int(got.totals[abi.SIP_SDPS]) == int(((gm["flags"] & SDP) != 0).sum()) == len(got.bodies())
    assert len(sc.run_reference(BY_NAME["spec_no_names"]).records()) == 0  # WANTED without a name wants nothing
    # capacities: the totals hold the full would-be values under every overflow
    m_, k_, nb, ns = sc.needs(BY_NAME["cap_exact"])
    assert ns > 1
    for name in ("cap_exact", "cap_spec_exact", "cap_no_text", "cap_roomy") + sc.OVERFLOWING:
        t = abi.sip_totals_dict(sc.run_reference(BY_NAME[name]).totals)
        assert (t["msgs"], t["fields"], t["text_bytes"], t["sdps"], t["overflow"]) == \
            (m_, k_, nb, ns, int(name in sc.OVERFLOWING)), name
    no_text, with_text = sc.run_reference(BY_NAME["cap_no_text"]), sc.run_reference(BY_NAME["cap_exact"])
    assert (no_text.records(k_) == with_text.records(k_)).all()  # positions and lengths without the text
    assert (no_text.messages(m_) == with_text.messages(m_)).all()


# ---------------------------------------------------------------- CPU: the reference's own vectors
def capture_case(b: PacketBatch, name: str, opts=None, **kw) -> sc.Case:
    """A capture through the parse's restatement: the records the device parse writes."""
    opts = opts or abi.make_opts()
    summary, layers = oracle.oracle_parse(b, opts)
    return sc.Case(name, np.concatenate([b.data, np.zeros(1, np.uint8)]), b.offsets, b.caplens, summary,
                   np.ascontiguousarray(layers).reshape(b.n, opts.max_layers), ml=opts.max_layers,
                   data_len=int(b.caplens.sum()), **kw)


_GOLDEN: dict = {}
ALL_FIELDS = dict(names=sc.NAMES, fields=abi.HTTP_FIELDS_ALL, text=3)


def frozen() -> dict:
    if "frozen" not in _GOLDEN:
        _GOLDEN["frozen"] = sc.load_frozen(VECTORS / "expected.npz")  # tools/make_golden_sip.py
    return _GOLDEN["frozen"]


def golden_batch(name: str) -> PacketBatch:
    if name not in _GOLDEN:
        _GOLDEN[name] = read_pcap(VECTORS / name)
    return _GOLDEN[name]


def golden_case(name: str) -> sc.Case:
    if ("case", name) not in _GOLDEN:
        _GOLDEN[("case", name)] = capture_case(golden_batch(name), name, **ALL_FIELDS)
    return _GOLDEN[("case", name)]


def frozen_rows(b: PacketBatch, msgs, fields, sdps, text) -> dict:
    """A call's records (every field, text 3) in the shape of expected.npz's entries, per source packet with a message.
    The version is reported as known or not (index 9), and a content length out of an int's range is None."""
    text = bytes(text)
    body = {int(s["msg"]): s for s in sdps}
    per = {}
    for j, m in enumerate(msgs):
        i, lo = int(m["index"]), int(m["layer_offset"])
        d = b.packet(i)[lo:lo + int(m["layer_len"])]
        pos, fl = int(m["text_pos"]), int(m["flags"])
        a = d[int(m["a_offset"]):int(m["a_offset"]) + int(m["a_len"])]
        assert text[pos:pos + int(m["a_len"])] == a
        rec = fields[int(m["first_field"]):int(m["first_field"]) + int(m["n_rec"])]
        assert len(rec) == int(m["n_fields"])
        rows = []
        for f in rec:
            no, vo = int(f["name_offset"]), int(f["value_offset"])
            rows.append([d[no:no + int(f["name_len"])].hex(), d[vo:vo + int(f["value_len"])].hex()])
            if int(f["name_id"]) != abi.HTTP_NO_NAME:
                tp = int(f["text_pos"])
                assert text[tp:tp + int(f["text_len"])] == d[vo:vo + int(f["value_len"])]
        s = body.get(j)
        assert (s is not None) == bool(fl & abi.SIP_HAS_SDP)
        per[i] = [int(m["kind"]), int(m["layer_len"]), int(m["header_len"]), int(m["n_fields"]), (fl >> 1) & 1,
                  None if fl & abi.SIP_CONTENT_LENGTH_RANGE else int(m["content_length"]), int(m["method"]), a.hex(),
                  int(m["status_code"]), bool(fl & abi.SIP_VERSION_KNOWN), int(m["first_line_len"]), fl & 1, rows,
                  None if s is None else [int(s["n_fields"]), bytes(s["owner_ipv4"]).hex(), int(s["audio_port"]),
                                          int(s["video_port"])]]
    return per


def assert_frozen(per: dict, disp, name: str, c: sc.Case) -> dict:
    """Exactly the packets the real reference builds a SIP layer in, and what it reports of each. A packet the contract
    leaves to the host is one whose chain the device did not finish, whose port gates another dissector, or whose
    answer is undefined in the reference; every undefined one is HOST."""
    want = frozen()[name]
    assert len(want) == golden_batch(name).n == len(disp)
    count = Counter()
    for i, w in enumerate(want):
        g, dv = per.get(i), int(disp[i])
        assert (g is not None) == (dv == sc.MSG)
        if w == "undefined":
            assert dv == sc.HOST, (name, i)
            count["undefined"] += 1
            continue
        if dv == sc.HOST:
            lay = sp.find_layer(golden_batch(name).packet(i), c.layers[i], int(c.summary["n_layers"][i]), c.ml,
                                int(c.summary["flags"][i]))
            assert lay == sp.HOST, (name, i)
            count["host"] += 1
            continue
        assert (g is None) == (w is None), (name, i, dv, w)
        if w is None:
            continue
        count["msgs"] += 1
        count["sdps"] += w[13] is not None
        w = list(w)
        w[9] = w[9] != ""
        if g[5] is None:
            w[5] = None
        assert g == w, (name, i, g[:12], w[:12])
    return count


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_reference_reproduces_the_real_sip_layers(name):
    """No packet is left out: a packet has a message exactly where the reference builds a SIP layer, with the same
    first line, fields and SDP answers; the undefined ones are HOST."""
    c = golden_case(name)
    got = sc.run_reference(c)
    t = abi.sip_totals_dict(got.totals)
    assert t["overflow"] == 0 and t["bad_desc"] == 0
    count = assert_frozen(frozen_rows(golden_batch(name), got.messages(), got.records(), got.bodies(), got.the_text()),
                          got.disposition[:c.n], name, c)
    assert count["msgs"] == t["msgs"] and count["sdps"] == t["sdps"]
    if name in REAL_FILES:
        assert count["undefined"] == 0
    else:
        assert 0 < count["undefined"] <= 0.05 * c.n and t["msgs"] >= 1500 and t["sdps"] >= 300
    if name == "packet_examples.pcap":
        assert (t["msgs"], t["sdps"], t["by_heuristic"], t["host_n"]) == (12, 5, 2, 2)
    sc.assert_same(got, sc.model(c), name)


def _calls_from_frozen(name: str, skip=()) -> dict:
    """sp.calls()'s table from the real layers' answers, without the packets in skip."""
    out: dict = {}
    esc = lambda h: bytes.fromhex(h).decode("latin-1").encode("unicode_escape").decode("ascii")  # noqa: E731
    for i, p in enumerate(frozen()[name]):
        if not isinstance(p, list) or i in skip:
            continue
        cid = [v for n_, v in p[12] if bytes.fromhex(n_).lower() == b"call-id"]
        c = out.setdefault(esc(cid[0]) if cid else "", {"packets": 0, "methods": Counter(), "status": Counter(),
                                                        "owners": set(), "audio_ports": set(), "video_ports": set()})
        c["packets"] += 1
        if p[0] == 0:
            c["methods"][abi.SIP_METHODS[p[6]]] += 1
        else:
            c["status"][str(p[8])] += 1
        if p[13] is not None:
            owner = bytes.fromhex(p[13][1])
            if owner != bytes(4):
                c["owners"].add(".".join(str(x) for x in owner))
            # (the reference reports 0 for a missing media line, and the example captures have no port 0)
            c["audio_ports"] |= {p[13][2]} - {0}
            c["video_ports"] |= {p[13][3]} - {0}
    return {k: {f: (dict(v) if isinstance(v, Counter) else sorted(v) if isinstance(v, set) else v)
                for f, v in c.items()} for k, c in out.items()}


def test_calls_gives_the_per_call_table():
    """calls() over the example captures equals the table worked out from the real layers' answers; the packets the
    contract leaves to the host (their chain stops before the carrier) are in neither."""
    name = "packet_examples.pcap"
    c = replace(golden_case(name), fields=abi.HTTP_FIELDS_WANTED)
    got = sc.run_reference(c)
    host = {i for i in range(c.n) if int(got.disposition[i]) == sc.HOST}
    tables = got.calls()
    assert tables == _calls_from_frozen(name, host) and len(host) == 2
    assert len(tables) >= 3 and sum(v["packets"] for v in tables.values()) == 12
    assert sum(1 for v in tables.values() if v["owners"] and v["audio_ports"]) >= 2


def _case_file(c: sc.Case, path: Path) -> None:
    want = sc.model(c)
    rec = sc.brief_of(c)[:c.n] if c.use_brief else c.summary
    spec = np.frombuffer(bytes(sc.spec_of(c)), np.uint8)
    head = np.array([c.n, c.dlen(), c.ml, 0 if c.use_brief else 1, c.maxm(), c.maxf(), c.maxs(), c.cap(),
                     int(c.want_text), int(c.want_disp)], np.uint64)
    parts = [head, spec, c.data[:c.dlen()], c.offsets, c.caplens, rec, c.layers, want.msgs[:c.maxm() * 48],
             want.fields[:c.maxf() * 24], want.sdps[:c.maxs() * 32]]
    parts += [want.text[:c.cap()]] if c.want_text else []
    parts += [want.disposition[:c.n]] if c.want_disp else []
    parts.append(want.totals)
    path.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))


def test_reference_under_sanitizers(tmp_path):
    """pcppx_sip_reference in a stand-alone program (its own main, host compiler, no HIP, nothing loaded into python)
    built with ASan + UBSan: the case families in exact-size heap buffers, the results equal to the model's."""
    gxx = shutil.which("g++")
    assert gxx is not None
    exe = tmp_path / "sip_ref_check"
    csrc = abi.PKG_DIR / "csrc"
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), "-I", str(csrc),
                    str(abi.REPO_DIR / "tests" / "native" / "sip_ref_check.cpp"),
                    str(csrc / "pcppx_sip_ref.cpp"), "-o", str(exe)], check=True)
    files = []
    for name in ("lines", "content", "fuzz", "fuzz_all", "ports", "long_names", "flags", "records", "cut_by_caplen",
                 "max_layers_1", "descriptors", "parsed_mixed", "n65_all", "n1025_1in100", "n2049_last", "n0_all",
                 "n65_brief", "spec_k1_f2_t3", "spec_k2_f1_t2", "spec_k3_f0_t1", "spec_no_names", "cap_exact",
                 "cap_msgs_short1", "cap_fields_short1", "cap_sdps_short1", "cap_text_short1", "cap_spec_short1",
                 "cap_no_text", "cap_sizing"):
        path = tmp_path / f"{name}.case"
        _case_file(BY_NAME[name], path)
        files.append(str(path))
    env = {"TMPDIR": str(tmp_path), "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(" ok\n") == len(files)


TOOL = [sys.executable, str(abi.REPO_DIR / "tools" / "sip_file.py")]


def test_sip_file_tool_without_gpu(tmp_path):
    """tools/sip_file.py --reference: the per-call table and the rows of a golden capture, without a GPU."""
    name = "packet_examples.pcap"
    c = replace(golden_case(name), fields=abi.HTTP_FIELDS_WANTED)
    want = sc.run_reference(c)
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "--calls"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert json.loads(run.stdout) == want.calls()
    out = tmp_path / "rows.txt"
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "-o", str(out)], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert out.read_text().split("\n") == [sp.format_row(r) for r in want.rows()] + [""]
    assert out.read_text().count("\n") >= 40


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_sip_equals_reference(engine, case):
    want = sc.run_reference(case)
    got = sc.run_device(engine, case)
    sc.assert_same(got, want, case.name)
    if case.name in sc.OVERFLOWING:
        sc.assert_untouched(got, case.name)


@pytest.mark.gpu
def test_gpu_sip_sizing_then_exact(engine):
    """The sizing call (no room at all) gives the four sizes; the call with exactly that room succeeds."""
    base = BY_NAME["cap_exact"]
    t = abi.sip_totals_dict(sc.run_device(engine, BY_NAME["cap_sizing"]).totals)
    assert t["overflow"] == 1
    exact = replace(base, out_msgs=t["msgs"], out_fields=t["fields"], out_sdps=t["sdps"], text_cap=t["text_bytes"])
    got = sc.run_device(engine, exact)
    assert int(got.totals[abi.SIP_OVERFLOW]) == 0
    sc.assert_same(got, sc.run_reference(exact), "exact")
    no_text = sc.run_device(engine, BY_NAME["cap_no_text"])
    assert (no_text.records(t["fields"]) == got.records(t["fields"])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1025_all", "n2049_1in100", "n2049_last", "spec_k2_f2_t3", "cap_sdps_short1",
                                  "cap_no_text"])
def test_gpu_sip_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = sc.run_reference(case)
    runs = [sc.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        sc.assert_same(r.result(), want, f"{name} run {k}")


@pytest.mark.gpu
def test_gpu_sip_source_on_both_sides_of_4gib(engine):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32
    (the layout of test_http.py's case): one SIP message lies across each line."""
    import torch

    import wide_cases as wc

    case = BY_NAME["n1025_all"]
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
    want = sc.run_reference(compact)
    assert int(want.totals[abi.SIP_MSGS]) >= n * 3 // 4
    assert {bool(o < wc.LINE) for o in wide.offsets} == {True, False}
    got = sc.run_device(engine, compact, source=source)
    sc.assert_same(got, want, "wide")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_gpu_golden_captures_from_a_device_parse(engine, name):
    """Parsed on the device, walked on the device: what the real SIP and SDP layers report; for the examples also the
    per-call table through tools/sip_file.py."""
    from pcapplusplus_amd.engine import sip_on_device

    b = golden_batch(name)
    spec = abi.make_sip_spec(sc.NAMES, abi.HTTP_FIELDS_ALL, 3)
    msgs, fields, sdps, text, disp, tot = sip_on_device(engine, b, spec)
    assert tot["msgs"] == len(msgs) == int((disp == abi.SIP_MSG).sum()) and tot["sdps"] == len(sdps)
    count = assert_frozen(frozen_rows(b, msgs, fields, sdps, text), disp, name, golden_case(name))
    assert count["msgs"] == tot["msgs"]
    if name != "packet_examples.pcap":
        return
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--calls"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    c = replace(golden_case(name), fields=abi.HTTP_FIELDS_WANTED)
    assert json.loads(run.stdout) == sc.run_reference(c).calls()
