"""pcppx_dhcp_device: the DHCP and DHCPv6 messages and their options of a device batch (include/pcppx.h, dhcp).

CPU: the ctypes mirrors match the header and every bad-argument family is refused before any device work;
pcppx_dhcp_reference (the contract in plain C++ over host pointers) equals pcapplusplus_amd.dhcp.model (the contract in
plain Python) on every case family of tests/dhcp_cases.py, byte for byte, the 0xA5 fill of everything else included (all
of it but the totals on overflow); the cases reach every rule and branch; the reference call reproduces what the real
DhcpLayer / DhcpV6Layer report on the reference's DHCP captures and on a crafted and mutated set
(tests/golden/dhcp/expected.npz, frozen by tools/make_golden_dhcp.py); leases() and fingerprints() read a crafted
exchange; and the reference call runs clean under ASan + UBSan in a stand-alone program.
GPU: pcppx_dhcp_device equals pcppx_dhcp_reference byte for byte on the same cases; two calls on two streams agree and
a repeat is bit-identical; a 66,561-packet batch (66 blocks); packets on both sides of offset 2^32; the golden captures
from a device parse.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import re
import shutil
import subprocess
import sys
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import dhcp_cases as dc
import oracle
from conftest import GOLDEN
from pcapplusplus_amd import abi
from pcapplusplus_amd import dhcp as dh
from pcapplusplus_amd.pcap import PacketBatch, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "dhcp"
CASES = dc.cases()
BY_NAME = {c.name: c for c in CASES}
GOLDEN_FILES = ("crafted.pcap", "packet_examples.pcap")


# ---------------------------------------------------------------- CPU: the ABI
def test_dhcp_structs_match_header():
    fields = {"pcppx_dhcp_spec": abi.DhcpSpec, "pcppx_dhcp_option": abi.DhcpOption, "pcppx_dhcp_msg": abi.DhcpMsg,
              "pcppx_dhcp_out": abi.DhcpOut}
    dtypes = {"pcppx_dhcp_msg": abi.DHCP_MSG_DTYPE, "pcppx_dhcp_option": abi.DHCP_OPTION_DTYPE}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = {"PCPPX_DHCP_NONE": abi.DHCP_NONE, "PCPPX_DHCP_MSG": abi.DHCP_MSG, "PCPPX_DHCP_HOST": abi.DHCP_HOST,
              "PCPPX_DHCP_BAD_DESC": abi.DHCP_BAD_DESC, "PCPPX_DHCP_V4": abi.DHCP_V4, "PCPPX_DHCP_V6": abi.DHCP_V6,
              "PCPPX_DHCP_OPTIONS_NONE": abi.DHCP_OPTIONS_NONE, "PCPPX_DHCP_OPTIONS_WANTED": abi.DHCP_OPTIONS_WANTED,
              "PCPPX_DHCP_OPTIONS_ALL": abi.DHCP_OPTIONS_ALL, "PCPPX_DHCP_MAX_CODES6": abi.DHCP_MAX_CODES6,
              "PCPPX_DHCP_HAS_MSG_TYPE": abi.DHCP_HAS_MSG_TYPE, "PCPPX_DHCP_HAS_MAC": abi.DHCP_HAS_MAC,
              "PCPPX_DHCP_MAGIC_OK": abi.DHCP_MAGIC_OK, "PCPPX_DHCP_HAS_LEASE_TIME": abi.DHCP_HAS_LEASE_TIME,
              "PCPPX_DHCP_HAS_SERVER_ID": abi.DHCP_HAS_SERVER_ID, "PCPPX_DHCP_REPLY": abi.DHCP_REPLY,
              "PCPPX_DHCP_MSGS": abi.DHCP_MSGS, "PCPPX_DHCP_V4_N": abi.DHCP_V4_N, "PCPPX_DHCP_V6_N": abi.DHCP_V6_N,
              "PCPPX_DHCP_OPTIONS": abi.DHCP_OPTIONS, "PCPPX_DHCP_VALUE_BYTES": abi.DHCP_VALUE_BYTES,
              "PCPPX_DHCP_HOST_N": abi.DHCP_HOST_N, "PCPPX_DHCP_BAD_DESC_N": abi.DHCP_BAD_DESC_N,
              "PCPPX_DHCP_OPTIONS_LINKED": abi.DHCP_OPTIONS_LINKED, "PCPPX_DHCP_REPLIES": abi.DHCP_REPLIES,
              "PCPPX_DHCP_OVERFLOW": abi.DHCP_OVERFLOW, "PCPPX_DHCP_TOTALS": abi.DHCP_TOTALS,
              "PCPPX_ABI_VERSION": abi.ABI_VERSION}
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu\\n", sizeof(pcppx_dhcp_spec), sizeof(pcppx_dhcp_option), sizeof(pcppx_dhcp_msg), '
           'sizeof(pcppx_dhcp_out));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(cls) for cls in fields.values()] == [72, 16, 80, 64]
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
    assert abi.ABI_VERSION == 7 and len(abi.DHCP_TOTAL_NAMES) == abi.DHCP_TOTALS


def test_dhcp_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_dhcp_device", "pcppx_dhcp_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_dhcp_spec()
    o = abi.DhcpOut(1, 1, 1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _want6(a, codes, n=None):
    a["s"] = abi.make_dhcp_spec(codes6=codes)
    if n is not None:
        a["s"].n_codes6 = n


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_msgs": lambda a: _set(a, "o", "msgs", None),
    "null_options": lambda a: _set(a, "o", "options", None),
    "reserved_set": lambda a: _set(a, "o", "reserved", 1),
    "reserved_high_bit": lambda a: _set(a, "o", "reserved", 1 << 63),
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
    "families_0": lambda a: _set(a, "s", "families", 0),
    "families_4": lambda a: _set(a, "s", "families", 4),
    "families_255": lambda a: _set(a, "s", "families", 255),
    "options_3": lambda a: _set(a, "s", "options", 3),
    "options_255": lambda a: _set(a, "s", "options", 255),
    "values_2": lambda a: _set(a, "s", "values", 2),
    "values_255": lambda a: _set(a, "s", "values", 255),
    "n_codes6_17": lambda a: _set(a, "s", "n_codes6", 17),
    "n_codes6_255": lambda a: _set(a, "s", "n_codes6", 255),
    "want6_equal": lambda a: _want6(a, (1, 3, 3)),
    "want6_descending": lambda a: _want6(a, (1, 3, 2, 39)),
    "want6_descending_last": lambda a: _want6(a, tuple(range(1, 16)) + (7,)),
    "want6_zero_after_first": lambda a: _want6(a, (5, 0)),
    "want6_beyond_n_codes6": lambda a: _want6(a, (1, 2, 3), 2),
    "want6_last_beyond": lambda a: _want6(a, (0,) * 15 + (9,), 0),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_dhcp_device's, pcppx_dhcp_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_dhcp_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_dhcp_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_dhcp_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_dhcp_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # a brief instead of the summary, absent optional outputs, an empty batch and the widest specs pass
    for name in ("n65_brief", "cap_no_values_no_disp", "n0_all", "spec_no_codes", "spec_16_codes6", "spec_codes_0_255"):
        assert int(dc.run_reference(BY_NAME[name]).totals[abi.DHCP_OVERFLOW]) == 0
    empty = dc.run_reference(BY_NAME["n0_all"])
    assert list(empty.totals) == [0] * abi.DHCP_TOTALS
    dc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_the_model(case):
    got = dc.run_reference(case)
    dc.assert_same(got, dc.model(case), case.name)
    if case.name in dc.OVERFLOWING:
        assert int(got.totals[abi.DHCP_OVERFLOW]) == 1
        dc.assert_untouched(got, case.name)
    else:
        assert int(got.totals[abi.DHCP_OVERFLOW]) == 0


def _disp(name: str) -> list:
    c = BY_NAME[name]
    return [int(d) for d in dc.run_reference(c).disposition[:c.n]]


def _by_packet(name: str, **kw):
    """(the case, its dispositions, its messages by source packet, its option records by source packet)."""
    c = replace(BY_NAME[name], **kw)
    got = dc.run_reference(c)
    msgs, recs = got.messages(), got.records()
    opts = {int(m["index"]): recs[int(m["first_option"]):int(m["first_option"]) + int(m["n_rec"])] for m in msgs}
    return c, [int(d) for d in got.disposition[:c.n]], {int(m["index"]): m for m in msgs}, opts


def test_cases_cover_the_contract():
    """The block size the cases are built around is the kernels', and the families reach the rules and branches they
    name: the values here are worked out by hand from the rules of include/pcppx.h."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kDhcpBlockPk\s*=\s*(\d+)", txt).group(1)) == dc.BLOCK
    assert max(c.n for c in CASES) <= 2100
    M, N, H, B = dc.MSG, dc.NONE, dc.HOST, dc.BAD
    MT, MAC, MAGIC, LT, SID, REPLY = (abi.DHCP_HAS_MSG_TYPE, abi.DHCP_HAS_MAC, abi.DHCP_MAGIC_OK,
                                      abi.DHCP_HAS_LEASE_TIME, abi.DHCP_HAS_SERVER_ID, abi.DHCP_REPLY)
    # rules 8, 9 and 11 with every option emitted
    c, d, m, o = _by_packet("walks")
    order = dc.WALK4 + dc.TYPED + dc.WALK6
    at = {("6_" if k >= len(dc.WALK4 + dc.TYPED) else "") + name: k for k, (name, _) in enumerate(order)}
    assert d == [M] * len(order)
    count = lambda name: (int(m[at[name]]["n_options"]), int(m[at[name]]["options_len"]))  # noqa: E731
    codes = lambda name: [(int(x["code"]), int(x["len"]), int(x["offset"])) for x in o[at[name]]]  # noqa: E731
    # rule 8: each stop condition
    assert count("L_240") == (0, 0) and int(m[at["L_240"]]["layer_len"]) == 240      # rem < 1 at once
    assert count("L_241_pad") == (1, 1) and codes("L_241_pad") == [(0, 0, 240)]
    assert count("L_241_end") == (1, 1) and codes("L_241_end") == [(255, 0, 240)]
    assert count("L_241_code") == (0, 0)                                              # rem < 2
    assert count("L_242_len_0") == (1, 2) and codes("L_242_len_0") == [(53, 0, 240)]
    assert count("L_242_len_1") == (0, 0)                                             # ends one byte behind L
    assert count("ends_at_L") == (1, 5) and codes("ends_at_L") == [(12, 3, 240)]
    assert count("ends_past_L") == (0, 0)
    assert count("ends_far_past_L") == (1, 3)
    assert count("len_255") == (2, 258) and codes("len_255") == [(43, 255, 240), (255, 0, 497)]
    assert count("end_then_pads") == (22, 24)                                         # END does not end the walk
    assert codes("end_then_options") == [(255, 0, 240), (53, 1, 241), (12, 4, 244), (255, 0, 250), (255, 0, 251)]
    assert int(m[at["end_then_options"]]["msg_type"]) == 5
    assert count("pads_between") == (9, 26)
    assert codes("code_0_and_255_with_lengths") == [(0, 0, 240), (5, 1, 241), (255, 0, 244)]  # then "03" alone
    assert count("code_0_and_255_with_lengths") == (3, 5)
    assert count("last_code_alone_behind_end") == (1, 1)
    # ordinals and value positions follow the walk
    x = o[at["end_then_options"]]
    assert [int(y["ordinal"]) for y in x] == [0, 1, 2, 3, 4] and [int(y["value_rel"]) for y in x] == [0, 0, 1, 5, 5]
    assert int(m[at["end_then_options"]]["value_len"]) == 5
    # rule 11: each typed value with len 0 / 3 / 4 / 5
    val = lambda name: (int(m[at[name]]["msg_type"]), int(m[at[name]]["lease_time"]),  # noqa: E731
                        bytes(m[at[name]]["server_id"]), int(m[at[name]]["flags"]) & (MT | LT | SID))
    Z = bytes(4)
    assert val("opt53_len0") == (0, 0, Z, MT) and val("opt53_len3") == (0x11, 0, Z, MT)
    assert val("opt53_len4") == (0x11, 0, Z, MT) and val("opt53_len5") == (0x11, 0, Z, MT)
    assert val("opt51_len0") == (0, 0, Z, 0) and val("opt51_len3") == (0, 0, Z, 0)
    assert val("opt51_len4") == (0, 0x11121314, Z, LT) and val("opt51_len5") == (0, 0x11121314, Z, LT)
    assert val("opt54_len0") == (0, 0, Z, 0) and val("opt54_len3") == (0, 0, Z, 0)
    assert val("opt54_len4") == (0, 0, bytes((0x11, 0x12, 0x13, 0x14)), SID) == val("opt54_len5")
    assert val("type_twice")[0] == 2 and val("type_first_empty") == (0, 0, Z, MT)      # the first option of a code
    assert val("lease_first_short") == (0, 0, Z, 0) and val("server_twice")[2] == bytes((1, 2, 3, 4))
    assert val("type_255")[0] == 255 and val("type_cut") == (0, 3600, Z, LT)
    fl = lambda name: int(m[at[name]]["flags"])  # noqa: E731
    mac = lambda name: bytes(m[at[name]]["client_mac"])  # noqa: E731
    assert fl("L_240") == MAC | MAGIC and mac("L_240") == bytes.fromhex("020000000001")
    assert fl("htype_6") == MAGIC and mac("htype_6") == bytes(6) and int(m[at["htype_6"]]["htype"]) == 6
    assert fl("hlen_16") == MAGIC and mac("hlen_16") == bytes(6) and fl("hlen_0") == MAGIC
    assert fl("bad_magic") == MAC | MT and fl("no_magic_all_ff") == 0 and count("no_magic_all_ff") == (60, 60)
    r = m[at["reply"]]
    assert fl("reply") == MAC | MAGIC | REPLY and fl("op_3") == MAC | MAGIC and int(r["op"]) == 2
    assert (int(r["secs"]), int(r["bootp_flags"]), int(r["hops"]), int(r["xid"])) == (0x1234, 0x8000, 3, 0x12345678)
    assert [bytes(r[f]) for f in ("ciaddr", "yiaddr", "siaddr", "giaddr")] == \
        [bytes((1, 2, 3, 4)), bytes((192, 168, 7, 9)), bytes((5, 6, 7, 8)), bytes((9, 10, 11, 12))]
    # rule 9: each stop condition, and DHCPv6's typed values
    assert count("6_L_4") == (0, 0) and count("6_L_5") == (0, 0) and count("6_L_7") == (0, 0)   # L - p < 4
    assert count("6_L_8_len_0") == (1, 4) and codes("6_L_8_len_0") == [(8, 0, 4)]
    assert count("6_L_8_len_1") == (0, 0) and count("6_ends_at_L") == (1, 10) and count("6_ends_past_L") == (0, 0)
    assert count("6_len_ffff") == (1, 6) and count("6_len_ffff_first") == (0, 0)
    assert codes("6_code_0_and_ffff") == [(0, 1, 4), (0xFFFF, 2, 9), (0x0100, 0, 15)]
    assert count("6_trailing_3") == (1, 5)
    t6 = lambda name: (int(m[at[name]]["msg_type"]), int(m[at[name]]["xid"]), int(m[at[name]]["family"]))  # noqa: E731
    assert t6("6_type_13") == (13, 0xABCDEF, 6) and t6("6_type_14") == (0, 0xABCDEF, 6)
    assert t6("6_type_0") == (0, 0xABCDEF, 6) and t6("6_type_255") == (0, 0xFFFFFF, 6)
    six = m[at["6_type_13"]]
    assert all(int(np.asarray(six[f]).sum()) == 0 for f in ("flags", "op", "htype", "hlen", "hops", "secs", "bootp_flags",
                                                            "lease_time", "ciaddr", "yiaddr", "client_mac", "server_id"))
    # WANTED picks by code: the same messages, fewer records
    _, _, wm, wo = _by_packet("walks_wanted")
    assert [int(x["code"]) for x in wo[at["pads_between"]]] == [53, 55] and int(wm[at["pads_between"]]["n_options"]) == 9
    assert [int(x["ordinal"]) for x in wo[at["pads_between"]]] == [2, 4]
    # rules 5 and 6
    pd = _disp("ports")
    np_, nq = len(dc.PORT_PAYLOADS), len(dc.PORTS)
    row = lambda name, base=0: pd[base + np_ * [n for n, _, _ in dc.PORTS].index(name):][:np_]  # noqa: E731
    V4, V6 = [M, M, N, N, N, N, N], [M, M, M, M, M, N, N]  # L >= 240; L >= 4
    for name in ("dhcp_68_67", "dhcp_67_68", "dhcp_67_67"):
        assert row(name) == V4, name
    for name in ("not_dhcp_68_68", "not_dhcp_67_40000", "not_dhcp_40000_67", "plain", "v6_to_vxlan", "v6_sip_src",
                 "v6_sips_dst"):
        assert row(name) == [N] * np_, name
    for name in ("v6_546_547", "v6_547_546", "v6_src_546", "v6_dst_547", "v6_src_547", "v6_dst_546", "v6_and_dhcp_port",
                 "v6_from_vxlan", "ntp_and_v6"):
        assert row(name) == V6, name
    for p in sorted(dh.HOST_OTHER_PORTS):
        assert row(f"v6_other_dst_{p}") == row(f"v6_other_src_{p}") == [H] * np_, p
    own = lambda name: row(name, np_ * nq)  # noqa: E731  the same packets under the parse's own flags
    assert own("dhcp_68_67") == V4 and own("v6_546_547") == V6 and own("plain") == [N] * np_
    assert own("v6_to_vxlan") == [H] * np_ and own("v6_other_dst_2152") == [H] * np_
    pm = {int(x["index"]): x for x in dc.run_reference(BY_NAME["ports"]).messages()}
    assert int(pm[0]["family"]) == 4 and int(pm[np_ * 6]["family"]) == 6 and int(pm[1]["layer_len"]) == 240
    # rules 2 and 3 over all flag combinations
    fl_ = _disp("flags")
    for k, f in enumerate(dc.flag_combinations()):
        host = f & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW) or \
            (f & abi.F_NEEDS_HOST_L7 and not f & abi.F_L7_KNOWN)
        none = not f & abi.F_NEEDS_HOST_L7 or f & (abi.F_L7_HTTP | abi.F_L7_SSL | abi.F_L7_DNS)
        assert fl_[k] == (H if host else N if none else M), hex(f)
    assert fl_.count(M) == 1
    # rule 4
    assert _disp("records") == [M, M, N, N, N, N, N, N, N, N, N, M, N, M, N, M, N, N, N, H, N, N]
    _, _, rm, _ = _by_packet("records")
    assert int(rm[1]["layer_len"]) == int(rm[0]["layer_len"]) - 4  # the trailer's bytes are not the message's
    assert int(rm[11]["layer_len"]) == 240 and int(rm[11]["n_options"]) == 0
    assert _disp("cut_by_caplen") == [M, N, N, N, N, M]
    assert set(_disp("max_layers_1")) == {H} and set(_disp("max_layers_2")) == {H} and set(_disp("max_layers_3")) == {M}
    dd = _disp("descriptors")
    assert [dd[i] for i in (5, 11, 17, 22, 30)] == [B] * 4 + [N]
    assert int(BY_NAME["descriptors"].offsets.max()) > 1 << 63  # the 64-bit wrap
    # the long walks
    t = abi.dhcp_totals_dict(dc.run_reference(BY_NAME["pads_1472"]).totals)
    assert (t["msgs"], t["options"], t["options_linked"], t["value_bytes"]) == (1, 1232, 1232, 0)
    big = dc.run_reference(BY_NAME["largest"])
    bm = big.messages()[0]
    assert int(BY_NAME["largest"].caplens[0]) == 65535 and int(bm["layer_len"]) == 65535 - 42
    assert int(bm["options_len"]) == 65535 - 42 - 240 and int(bm["n_options"]) == int(bm["n_rec"]) > 20000
    assert int(big.records()[-1]["code"]) == 255 and int(big.records()[-1]["offset"]) == 65535 - 42 - 1
    # every disposition, flag and family is reached
    alive = [c for c in CASES if c.name not in dc.OVERFLOWING]
    allm = np.concatenate([dc.run_reference(c).messages() for c in alive])
    bits = 0
    for f in {int(x) for x in allm["flags"]}:
        bits |= f
    assert bits == 63 and {int(x) for x in allm["family"]} == {4, 6}
    assert {int(x) for x in allm["msg_type"][allm["family"] == 6]} >= set(range(14))
    seen = set()
    for c in alive:
        if c.want_disp:
            seen |= set(_disp(c.name))
    assert seen == {N, M, H, B}
    # the parse's own records find the messages
    pt = abi.dhcp_totals_dict(dc.run_reference(BY_NAME["parsed_mixed"]).totals)
    assert pt["v4"] >= 150 and pt["v6"] >= 80
    assert pt["host_n"] == 2 * len(dh.HOST_OTHER_PORTS) * len(dc.PORT_PAYLOADS)  # rule 6's rows; nothing else is HOST
    assert abi.dhcp_totals_dict(dc.run_reference(BY_NAME["parsed_ml2"]).totals)["host_n"] == 64
    # batch shapes
    for n in dc.SIZES:
        t = {share: abi.dhcp_totals_dict(dc.run_reference(BY_NAME[f"n{n}_{share}"]).totals) for share in dc.SHARES}
        assert t["last"]["msgs"] == (1 if n else 0) and t["1in100"]["msgs"] == len(range(0, n, 100))
        assert t["all"]["msgs"] == n and (n < 3 or (t["all"]["v4"] and t["all"]["v6"] and t["all"]["replies"]))
        if n:
            assert _disp(f"n{n}_last")[-1] == M
    # families choose the messages; options and values choose the records and the bytes, never the messages' own values
    fm = dc.run_reference(BY_NAME["spec_f3_o2_v1"]).messages()
    for families in (1, 2, 3):
        for options in (0, 1, 2):
            for values in (0, 1):
                got = dc.run_reference(BY_NAME[f"spec_f{families}_o{options}_v{values}"])
                gm, gr = got.messages(), got.records()
                keep = fm[[bool(families & (1 if int(x) == 4 else 2)) for x in fm["family"]]]
                for f in ("index", "xid", "lease_time", "layer_len", "n_options", "options_len", "family", "msg_type",
                          "flags", "client_mac", "server_id", "yiaddr"):
                    assert (gm[f] == keep[f]).all(), (families, options, values, f)
                assert (options == 0) == (len(gr) == 0)
                if options == 2:
                    assert len(gr) == int(gm["n_options"].sum())
                assert int(got.totals[abi.DHCP_VALUE_BYTES]) == (int(gr["len"].sum()) if values else 0) == \
                    int(gm["value_len"].sum())
    assert len(dc.run_reference(BY_NAME["spec_no_codes"]).records()) == 0  # WANTED without a code wants nothing
    r0 = dc.run_reference(BY_NAME["spec_codes_0_255"]).records()
    assert {int(x) for x in r0["code"]} == {0, 255} and (r0["len"] == 0).sum() < len(r0)  # v4 PAD / END and v6 code 0
    r16 = dc.run_reference(BY_NAME["spec_16_codes6"])
    six = {int(j) for j, x in enumerate(r16.messages()) if int(x["family"]) == 6}
    got6 = {int(x["code"]) for x in r16.records() if int(x["msg"]) in six}
    assert got6 <= set(dc.CODES6_16) and {1, 3, 6, 8, 39, 0x0100, 0xFFFF} <= got6
    # capacities: the totals hold the full would-be values under every overflow
    m_, k_, nb = dc.needs(BY_NAME["cap_exact"])
    assert m_ > 1 and k_ > 1 and nb > 1
    for name in ("cap_exact", "cap_spec_exact", "cap_no_values", "cap_roomy") + dc.OVERFLOWING:
        t = abi.dhcp_totals_dict(dc.run_reference(BY_NAME[name]).totals)
        assert (t["msgs"], t["options"], t["value_bytes"], t["overflow"]) == \
            (m_, k_, nb, int(name in dc.OVERFLOWING)), name
    no_values, with_values = dc.run_reference(BY_NAME["cap_no_values"]), dc.run_reference(BY_NAME["cap_exact"])
    assert (no_values.records(k_) == with_values.records(k_)).all()  # positions and lengths without the bytes
    assert (no_values.messages(m_) == with_values.messages(m_)).all()


# ---------------------------------------------------------------- CPU: the tables
def test_leases_and_fingerprints_on_a_dora_exchange():
    """discover, offer, request, ack of three clients, the second without a host name, the third renamed between its
    DISCOVER and its REQUEST; a DHCPv6 message in between."""
    pk = dc.dora(1) + dc.dora(2, b"")[:1] + [dh.packet(dc.solicit(3), 9, 546, 547)] + dc.dora(2, b"")[1:]
    third = dc.dora(3)
    third[2] = dh.packet(dc.request(3, b"renamed\0x"), 14)
    got = dc.run_reference(dc.make("dora", pk + third))
    assert int(got.totals[abi.DHCP_MSGS]) == 13 and int(got.totals[abi.DHCP_V6_N]) == 1
    assert got.leases() == [
        {"index": 3, "client_mac": "02:00:00:00:00:01", "yiaddr": "10.0.0.1", "lease_time": 86401,
         "server_id": "10.0.0.1", "host_name": "host-1"},
        {"index": 8, "client_mac": "02:00:00:00:00:02", "yiaddr": "10.0.0.2", "lease_time": 86402,
         "server_id": "10.0.0.1", "host_name": ""},
        {"index": 12, "client_mac": "02:00:00:00:00:03", "yiaddr": "10.0.0.3", "lease_time": 86403,
         "server_id": "10.0.0.1", "host_name": "renamed\\x00x"}]
    fp = got.fingerprints()
    assert [(f["index"], f["msg_type"]) for f in fp] == [(0, 1), (2, 3), (4, 1), (7, 3), (9, 1), (11, 3)]
    assert fp[0] == {"index": 0, "client_mac": "02:00:00:00:00:01", "msg_type": dh.DISCOVER,
                     "params": list(dc.PARAMS), "vendor": "MSFT 5.0"}
    assert fp[1]["params"] == list(dc.PARAMS[:9]) and fp[1]["vendor"] is None
    rows = got.rows()
    assert rows[0] == (0, 4, 1, None, 6, b"") and rows[1] == (0, 4, 1, 53, 1, b"\x01")
    assert (0, 4, 1, 12, 6, b"host-1") in rows and len(rows) == 13 + int(got.totals[abi.DHCP_OPTIONS])
    assert dh.format_row(rows[1]) == "0 v4 type=1 opt=53 len=1 01" and dh.format_row(rows[0]) == "0 v4 type=1 options=6"


# ---------------------------------------------------------------- CPU: the reference's own vectors
def capture_case(b: PacketBatch, name: str, opts=None, **kw) -> dc.Case:
    """A capture through the parse's restatement: the records the device parse writes."""
    opts = opts or abi.make_opts()
    summary, layers = oracle.oracle_parse(b, opts)
    return dc.Case(name, np.concatenate([b.data, np.zeros(1, np.uint8)]), b.offsets, b.caplens, summary,
                   np.ascontiguousarray(layers).reshape(b.n, opts.max_layers), ml=opts.max_layers,
                   data_len=int(b.caplens.sum()), **kw)


@functools.lru_cache(maxsize=None)
def frozen() -> dict:
    return dc.load_frozen(VECTORS / "expected.npz")  # tools/make_golden_dhcp.py


@functools.lru_cache(maxsize=None)
def golden_batch(name: str) -> PacketBatch:
    return read_pcap(VECTORS / name)


@functools.lru_cache(maxsize=None)
def golden_case(name: str) -> dc.Case:
    return capture_case(golden_batch(name), name, options=dc.ALL, values=1)


def frozen_rows(b: PacketBatch, msgs, options, values) -> dict:
    """A call's records (every option, with values) in the shape of expected.npz's entries, per source packet with a
    message."""
    values = bytes(values)
    per = {}
    for m in msgs:
        i, lo = int(m["index"]), int(m["layer_offset"])
        d = b.packet(i)[lo:lo + int(m["layer_len"])]
        rec = options[int(m["first_option"]):int(m["first_option"]) + int(m["n_rec"])]
        assert len(rec) == int(m["n_options"]) and [int(r["ordinal"]) for r in rec] == list(range(len(rec)))
        rows = []
        for r in rec:
            at = int(m["value_pos"]) + int(r["value_rel"])
            v = values[at:at + int(r["len"])]
            head = 4 if int(m["family"]) == 6 else 1 if int(r["code"]) in (0, 255) else 2
            assert v == d[int(r["offset"]) + head:int(r["offset"]) + head + int(r["len"])]
            rows.append([int(r["code"]), int(r["len"]), v.hex()])
        if int(m["family"]) == 4:
            hdr = [int(m["op"])] + [bytes(m[f]).hex() for f in ("ciaddr", "yiaddr", "siaddr", "giaddr", "client_mac")] + \
                [int(m["xid"]), int(m["secs"]), int(m["bootp_flags"])]
        else:
            hdr = [int(m["xid"])]
        per[i] = [int(m["family"]), int(m["layer_len"]), int(m["msg_type"]), int(m["n_options"]), hdr, rows]
    return per


def assert_frozen(per: dict, disp, name: str, c: dc.Case) -> dict:
    """Exactly the packets the real reference builds a DHCP / DHCPv6 layer in, and what it reports of each. A packet
    the contract leaves to the host is one whose chain the device did not finish or whose other port gates RADIUS or
    GTP."""
    want = frozen()[name]
    assert len(want) == golden_batch(name).n == len(disp)
    count = {"v4": 0, "v6": 0, "host": 0}
    for i, w in enumerate(want):
        g, dv = per.get(i), int(disp[i])
        assert (g is not None) == (dv == dc.MSG)
        if dv == dc.HOST:
            lay = dh.find_layer(golden_batch(name).packet(i), c.layers[i], int(c.summary["n_layers"][i]), c.ml,
                                int(c.summary["flags"][i]))
            assert lay == dh.HOST, (name, i)
            count["host"] += 1
            continue
        assert (g is None) == (w is None), (name, i, dv, w)
        if w is None:
            continue
        count["v4" if w[0] == 4 else "v6"] += 1
        assert g == w, (name, i, g[:5], w[:5])
    return count


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_reference_reproduces_the_real_dhcp_layers(name):
    """No packet is left out: a packet has a message exactly where the reference builds a DhcpLayer or a DhcpV6Layer,
    with the same header getters, message type, option count and options."""
    c = golden_case(name)
    got = dc.run_reference(c)
    t = abi.dhcp_totals_dict(got.totals)
    assert t["overflow"] == 0 and t["bad_desc"] == 0
    count = assert_frozen(frozen_rows(golden_batch(name), got.messages(), got.records(), got.the_values()),
                          got.disposition[:c.n], name, c)
    assert (count["v4"], count["v6"]) == (t["v4"], t["v6"])
    if name == "crafted.pcap":
        assert t["msgs"] >= c.n // 2 and t["v4"] >= 100 and t["v6"] >= 100
    else:
        assert t["v4"] >= 4 and t["v6"] >= 6 and count["host"] <= t["host_n"]
        d3 = [m for m in got.messages() if int(m["n_options"]) == 232]  # Dhcp3.pcap: trailing PADs, each an option
        assert d3 and int(got.records()[int(d3[0]["first_option"]) + 231]["code"]) == 0
    dc.assert_same(got, dc.model(c), name)


def _case_file(c: dc.Case, path: Path) -> None:
    want = dc.model(c)
    rec = dc.brief_of(c)[:c.n] if c.use_brief else c.summary
    spec = np.frombuffer(bytes(dc.spec_of(c)), np.uint8)
    head = np.array([c.n, c.dlen(), c.ml, 0 if c.use_brief else 1, c.maxm(), c.maxo(), c.cap(), int(c.want_values),
                     int(c.want_disp)], np.uint64)
    parts = [head, spec, c.data[:c.dlen()], c.offsets, c.caplens, rec, c.layers, want.msgs[:c.maxm() * 80],
             want.options[:c.maxo() * 16]]
    parts += [want.values[:c.cap()]] if c.want_values else []
    parts += [want.disposition[:c.n]] if c.want_disp else []
    parts.append(want.totals)
    path.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))


def test_reference_under_sanitizers(tmp_path):
    """pcppx_dhcp_reference in a stand-alone program (its own main, host compiler, no HIP, nothing loaded into python)
    built with ASan + UBSan: the case families in exact-size heap buffers, the results equal to the model's."""
    gxx = shutil.which("g++")
    assert gxx is not None
    exe = tmp_path / "dhcp_ref_check"
    csrc = abi.PKG_DIR / "csrc"
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), "-I", str(csrc),
                    str(abi.REPO_DIR / "tests" / "native" / "dhcp_ref_check.cpp"),
                    str(csrc / "pcppx_dhcp_ref.cpp"), "-o", str(exe)], check=True)
    files = []
    for name in ("walks", "walks_wanted", "fuzz", "fuzz_all", "ports", "pads_1472", "largest", "flags", "records",
                 "cut_by_caplen", "max_layers_1", "descriptors", "parsed_mixed", "n65_all", "n1025_1in100",
                 "n2049_last", "n0_all", "n65_brief", "spec_f1_o2_v1", "spec_f2_o1_v0", "spec_f3_o0_v1",
                 "spec_codes_0_255", "spec_16_codes6", "cap_exact", "cap_msgs_short1", "cap_options_short1",
                 "cap_values_short1", "cap_spec_short1", "cap_no_values", "cap_sizing"):
        path = tmp_path / f"{name}.case"
        _case_file(BY_NAME[name], path)
        files.append(str(path))
    env = {"TMPDIR": str(tmp_path), "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(" ok\n") == len(files)


TOOL = [sys.executable, str(abi.REPO_DIR / "tools" / "dhcp_file.py")]


def test_dhcp_file_tool_without_gpu(tmp_path):
    """tools/dhcp_file.py --reference: the lease table and the rows of a golden capture, without a GPU."""
    name = "packet_examples.pcap"
    c = replace(golden_case(name), options=dc.WANTED)
    want = dc.run_reference(c)
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "--leases"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert json.loads(run.stdout) == want.leases() and len(want.leases()) >= 1
    out = tmp_path / "rows.txt"
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "-o", str(out)], capture_output=True,
                         text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert out.read_text().split("\n") == [dh.format_row(r) for r in want.rows()] + [""]
    assert out.read_text().count("\n") >= 30


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_dhcp_equals_reference(engine, case):
    want = dc.run_reference(case)
    got = dc.run_device(engine, case)
    dc.assert_same(got, want, case.name)
    if case.name in dc.OVERFLOWING:
        dc.assert_untouched(got, case.name)


@pytest.mark.gpu
def test_gpu_dhcp_sizing_then_exact(engine):
    """The sizing call (no room at all) gives the three sizes; the call with exactly that room succeeds."""
    base = BY_NAME["cap_exact"]
    t = abi.dhcp_totals_dict(dc.run_device(engine, BY_NAME["cap_sizing"]).totals)
    assert t["overflow"] == 1
    exact = replace(base, out_msgs=t["msgs"], out_options=t["options"], values_cap=t["value_bytes"])
    got = dc.run_device(engine, exact)
    assert int(got.totals[abi.DHCP_OVERFLOW]) == 0
    dc.assert_same(got, dc.run_reference(exact), "exact")
    no_values = dc.run_device(engine, BY_NAME["cap_no_values"])
    assert (no_values.records(t["options"]) == got.records(t["options"])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1025_all", "n2049_1in100", "n2049_last", "spec_f2_o2_v1", "cap_options_short1",
                                  "cap_no_values"])
def test_gpu_dhcp_is_repeatable_across_streams(engine, name):
    import torch

    case = BY_NAME[name]
    want = dc.run_reference(case)
    runs = [dc.DeviceRun(case) for _ in range(3)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for r, s in zip(runs, streams):  # two calls in flight on two streams: the context's scratch orders them
        r.launch(engine, s.cuda_stream)
    torch.cuda.synchronize()
    runs[2].launch(engine, torch.cuda.current_stream().cuda_stream)  # and a repeat
    for k, r in enumerate(runs):
        dc.assert_same(r.result(), want, f"{name} run {k}")


N_WIDE, STEP = 66561, 64  # 65 blocks of 1024 and one packet; blocks a step of the base kernel
WIDE_TOTALS = {"msgs": 666, "options": 2860, "value_bytes": 25314}  # frozen; none is zero: every scanned carry is used


@functools.lru_cache(maxsize=None)
def wide():
    """(the 66-block case, what the reference leaves): built once, shared by the CPU and the GPU test."""
    case = dc.make("wide", dc.mixed(N_WIDE, "1in100"))
    return case, dc.run_reference(case)


def test_reference_past_64_blocks():
    case, want = wide()
    assert case.n == N_WIDE and (N_WIDE + dc.BLOCK - 1) // dc.BLOCK == STEP + 2
    dc.assert_same(want, dc.model(case), "wide")
    totals = abi.dhcp_totals_dict(want.totals)
    assert totals["overflow"] == 0 and totals["host_n"] == 0 and totals["bad_desc"] == 0
    disp = want.disposition[:N_WIDE]
    assert int((disp[STEP * dc.BLOCK:(STEP + 1) * dc.BLOCK] == dc.MSG).sum()) >= 1, "block 64 holds no message"
    assert int((disp[:STEP * dc.BLOCK] == dc.MSG).sum()) >= 1
    assert all(v != 0 for v in WIDE_TOTALS.values()) and {k: totals[k] for k in WIDE_TOTALS} == WIDE_TOTALS


@pytest.mark.gpu
def test_gpu_dhcp_past_64_blocks(engine):
    case, want = wide()
    dc.assert_same(dc.run_device(engine, case), want, "wide")


@pytest.mark.gpu
def test_gpu_dhcp_source_on_both_sides_of_4gib(engine):
    """The packets of n1025_all laid around offset 2^32 and around the offset whose address is a multiple of 2^32
    (the layout of test_http.py's case): one message lies across each line."""
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
    wide_, compact = perm(case, offs), perm(case, case.offsets)
    source = (data, torch.from_numpy(wide_.offsets.view(np.int64)).to("cuda:0"),
              torch.from_numpy(wide_.caplens.view(np.int32)).to("cuda:0"), lay.data_len)
    want = dc.run_reference(compact)
    assert int(want.totals[abi.DHCP_MSGS]) == n
    assert {bool(o < wc.LINE) for o in wide_.offsets} == {True, False}
    got = dc.run_device(engine, compact, source=source)
    dc.assert_same(got, want, "wide")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_gpu_golden_captures_from_a_device_parse(engine, name):
    """Parsed on the device, walked on the device: what the real DhcpLayer and DhcpV6Layer report."""
    from pcapplusplus_amd.engine import dhcp_on_device

    b = golden_batch(name)
    spec = abi.make_dhcp_spec(options=dc.ALL, values=1)
    msgs, options, values, disp, tot = dhcp_on_device(engine, b, spec)
    assert tot["msgs"] == len(msgs) == int((disp == abi.DHCP_MSG).sum()) and tot["options"] == len(options)
    count = assert_frozen(frozen_rows(b, msgs, options, values), disp, name, golden_case(name))
    assert count["v4"] + count["v6"] == tot["msgs"]
