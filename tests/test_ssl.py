"""pcppx_ssl_device: the SSL/TLS records, the hellos and the SNI of the SSL packets of a device batch (include/pcppx.h,
ssl).

CPU: the ctypes mirrors match the header and every bad-argument family is refused before any device work;
pcppx_ssl_reference (the contract in plain C++ over host pointers) equals pcapplusplus_amd.ssl.model (the contract in
plain Python over byte slices) on every case family of tests/ssl_cases.py, byte for byte, the 0xA5 fill of everything else
included (all of it but the totals on overflow); it reproduces what the real SSLLayer / SSLClientHelloMessage /
SSLServerHelloMessage report on the reference's SSL captures and on a crafted and mutated set
(tests/golden/ssl/expected.npz, frozen by tools/make_golden_ssl.py); analyze() reproduces the two reports the reference's
SSLAnalyzer test expects; and the reference call runs clean under ASan + UBSan in a stand-alone program.
GPU: pcppx_ssl_device equals pcppx_ssl_reference byte for byte on the same cases; two calls on two streams agree and a
repeat is bit-identical; SSL packets on both sides of offset 2^32; the golden captures from a device parse.
"""
from __future__ import annotations

import ctypes as C
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

import oracle
import ssl_cases as sc
from conftest import GOLDEN
from pcapplusplus_amd import abi
from pcapplusplus_amd import ssl as sl
from pcapplusplus_amd.pcap import PacketBatch, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "ssl"
CASES = sc.cases()
BY_NAME = {c.name: c for c in CASES}
REPORTS = {"tls.pcap": "sslanalyzer_tls.txt", "many_protocols_ssl.pcap": "sslanalyzer_manyprotocols.txt"}
# the names in the two reports, from the IANA TLS registries (cipher suites; the protocol versions of RFC 2246, 5246, 8446)
IANA_SUITES = {"TLS_RSA_WITH_RC4_128_SHA": 0x0005, "TLS_RSA_WITH_AES_128_CBC_SHA": 0x002F,
               "TLS_DHE_RSA_WITH_AES_128_CBC_SHA": 0x0033, "TLS_AES_128_GCM_SHA256": 0x1301,
               "TLS_ECDHE_ECDSA_WITH_AES_128_GCM_SHA256": 0xC02B, "TLS_ECDHE_RSA_WITH_AES_128_GCM_SHA256": 0xC02F}
VERSIONS = {"TLS 1.0": 0x0301, "TLS 1.2": 0x0303, "TLS 1.3": 0x0304}


# ---------------------------------------------------------------- CPU: the ABI
def test_ssl_structs_match_header():
    fields = {"pcppx_ssl_spec": abi.SslSpec, "pcppx_ssl_msg": abi.SslMsg, "pcppx_ssl_hello": abi.SslHello,
              "pcppx_ssl_out": abi.SslOut}
    dtypes = {"pcppx_ssl_msg": abi.SSL_MSG_DTYPE, "pcppx_ssl_hello": abi.SSL_HELLO_DTYPE}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = {"PCPPX_SSL_NONE": abi.SSL_NONE, "PCPPX_SSL_MSG": abi.SSL_MSG, "PCPPX_SSL_HOST": abi.SSL_HOST,
              "PCPPX_SSL_BAD_DESC": abi.SSL_BAD_DESC, "PCPPX_SSL_CLIENT": abi.SSL_CLIENT,
              "PCPPX_SSL_SERVER": abi.SSL_SERVER, "PCPPX_SSL_KIND_CLIENT": abi.SSL_KIND_CLIENT,
              "PCPPX_SSL_KIND_SERVER": abi.SSL_KIND_SERVER, "PCPPX_SSL_NO_TCP": abi.SSL_NO_TCP,
              "PCPPX_SSL_HAS_SNI": abi.SSL_HAS_SNI, "PCPPX_SSL_SNI_TRUNCATED": abi.SSL_SNI_TRUNCATED,
              "PCPPX_SSL_SNI_MALFORMED": abi.SSL_SNI_MALFORMED, "PCPPX_SSL_HAS_CIPHER": abi.SSL_HAS_CIPHER,
              "PCPPX_SSL_MSGS": abi.SSL_MSGS, "PCPPX_SSL_HELLOS": abi.SSL_HELLOS,
              "PCPPX_SSL_CLIENT_HELLOS": abi.SSL_CLIENT_HELLOS, "PCPPX_SSL_SERVER_HELLOS": abi.SSL_SERVER_HELLOS,
              "PCPPX_SSL_NAME_BYTES": abi.SSL_NAME_BYTES, "PCPPX_SSL_HOST_N": abi.SSL_HOST_N,
              "PCPPX_SSL_BAD_DESC_N": abi.SSL_BAD_DESC_N, "PCPPX_SSL_PAYLOAD_BYTES": abi.SSL_PAYLOAD_BYTES,
              "PCPPX_SSL_ALERT_PKTS": abi.SSL_ALERT_PKTS, "PCPPX_SSL_APPDATA_PKTS": abi.SSL_APPDATA_PKTS,
              "PCPPX_SSL_OVERFLOW": abi.SSL_OVERFLOW, "PCPPX_SSL_TOTALS": abi.SSL_TOTALS,
              "PCPPX_ABI_VERSION": abi.ABI_VERSION}
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu %zu\\n", sizeof(pcppx_ssl_spec), sizeof(pcppx_ssl_msg), sizeof(pcppx_ssl_hello), '
           'sizeof(pcppx_ssl_out));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(cls) for cls in fields.values()] == [8, 32, 32, 56]
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
    assert abi.ABI_VERSION == 7 and len(abi.SSL_TOTAL_NAMES) == abi.SSL_TOTALS
    assert re.search(r"static_assert\(sizeof\(Plan\) == 16", (abi.PKG_DIR / "csrc" / "pcppx_ssl.hip").read_text())


def test_ssl_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_ssl_device", "pcppx_ssl_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_ssl_spec()
    o = abi.SslOut(1, 1, 1, 1, 1, 1, 1, 1)
    return dict(b=b, r=r, ml=6, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _reserved(a, k):
    a["s"].reserved[k] = 1


BAD_ARGS = {
    "null_totals": lambda a: _set(a, "o", "totals", None),
    "null_msgs": lambda a: _set(a, "o", "msgs", None),
    "null_hellos": lambda a: _set(a, "o", "hellos", None),
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
    "kinds_4": lambda a: _set(a, "s", "kinds", 4),
    "kinds_255": lambda a: _set(a, "s", "kinds", 255),
    "reserved_0": lambda a: _reserved(a, 0),
    "reserved_1": lambda a: _reserved(a, 1),
    "reserved_2": lambda a: _reserved(a, 2),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_ssl_device's, pcppx_ssl_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_ssl_device(ctx, ref("b"), ref("r"), a["ml"], ref("s"), ref("o"), None)
    host = None if ctx is None else lib.pcppx_ssl_reference(ref("b"), ref("r"), a["ml"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_ssl_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_ssl_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # kinds 0, a brief instead of the summary, absent optional outputs and an empty batch pass
    for name in ("kinds_0", "n65_brief", "cap_no_names_no_disp", "n0"):
        assert int(sc.run_reference(BY_NAME[name]).totals[abi.SSL_OVERFLOW]) == 0
    empty = sc.run_reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.SSL_TOTALS
    sc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_the_model(case):
    got = sc.run_reference(case)
    sc.assert_same(got, sc.model(case), case.name)
    if case.name in sc.OVERFLOWING:
        assert int(got.totals[abi.SSL_OVERFLOW]) == 1
        sc.assert_untouched(got, case.name)
    else:
        assert int(got.totals[abi.SSL_OVERFLOW]) == 0


def _disp(name: str) -> list:
    c = BY_NAME[name]
    return [int(d) for d in sc.run_reference(c).disposition[:c.n]]


def _hellos_by_packet(got: sc.Buffers) -> dict:
    """source packet -> [(kind, version, cipher, n_ciphers, n_ext, sid, flags, name), ...]"""
    out: dict = {}
    for r in got.rows():
        out.setdefault(r[0], []).append(r[1:])
    return out


def test_cases_cover_the_contract():
    """The block size the cases are built around is the kernels', and the families reach the paths they name: the
    values here are worked out by hand from the rules of include/pcppx.h."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kSslBlockPk\s*=\s*(\d+)", txt).group(1)) == sc.BLOCK
    assert max(c.n for c in CASES) <= 2100
    SNI, TR, MAL, HC = abi.SSL_HAS_SNI, abi.SSL_SNI_TRUNCATED, abi.SSL_SNI_MALFORMED, abi.SSL_HAS_CIPHER
    CL, SV = abi.SSL_CLIENT, abi.SSL_SERVER
    # rule 3: the record-type mix
    rt = sc.run_reference(BY_NAME["record_types"])
    m = {name: rt.messages()[k] for k, (name, _) in enumerate(sc.RECORD_TYPES)}
    mix = lambda x: tuple(int(x[f]) for f in ("n_handshake", "n_ccs", "n_alert", "n_appdata", "n_hellos"))  # noqa: E731
    assert mix(m["ccs"]) == (0, 1, 0, 0, 0) and mix(m["alert"]) == (0, 0, 1, 0, 0)
    assert mix(m["handshake_client"]) == (1, 0, 0, 0, 1) and mix(m["appdata"]) == (0, 0, 0, 1, 0)
    assert mix(m["server_flight"]) == (3, 0, 0, 0, 1) and mix(m["client_finish"]) == (2, 1, 0, 0, 0)
    assert mix(m["all_four"]) == (1, 1, 1, 2, 1) and mix(m["record_cut"]) == (0, 0, 0, 1, 0)
    assert int(m["appdata"]["payload_len"]) == 105 and int(m["appdata"]["layer_offset"]) == sc.AT
    assert (int(m["appdata"]["src_port"]), int(m["appdata"]["dst_port"]), int(m["appdata"]["ssl_port"])) == (40004, 443, 443)
    assert (int(m["handshake_server"]["src_port"]), int(m["handshake_server"]["ssl_port"])) == (443, 443)
    t = abi.ssl_totals_dict(rt.totals)
    assert (t["alert_pkts"], t["appdata_pkts"], t["client_hellos"], t["server_hellos"]) == (3, 5, 3, 2)
    assert t["payload_bytes"] == int(rt.messages()["payload_len"].sum())
    # rules 4-7, one hello case a packet
    by = _hellos_by_packet(sc.run_reference(BY_NAME["hellos"]))
    h = {name: by.get(k, []) for k, (name, _) in enumerate(sc.HELLOS)}
    kinds = lambda name: [x[0] for x in h[name]]  # noqa: E731
    assert h["client_plain"] == [(CL, 0x0303, 0, 3, 3, 0, SNI, b"www.example.org")]
    assert h["server_plain"] == [(SV, 0x0303, 0xC02F, 0, 1, 0, HC, b"")]
    assert h["server_tls13"] == [(SV, 0x0304, 0x1301, 0, 2, 32, HC, b"")]
    assert kinds("both_client_first") == [CL, SV] and kinds("both_server_first") == [SV, CL]
    assert [x[7] for x in h["two_clients"]] == [b"first"]
    for name in ("behind_type_8", "behind_type_22", "behind_type_3", "behind_type_255"):  # rule 4 (b)
        assert h[name] == [], name
    assert kinds("behind_hello_request") == [CL] and kinds("behind_certificate") == [SV] and kinds("behind_finished") == [CL]
    assert kinds("five_zeros_D15") == [CL] and h["five_zeros_D15"][0][1] == 0x0303 and h["five_zeros_D16"] == []
    assert kinds("byte1_D15") == [CL] and h["byte1_D15"][0][1] == 0x0301 and h["byte1_D16"] == [] and h["byte1_behind"] == []
    assert h["D_3"] == [] and h["D_4"] == [(CL, 0, 0, 0, 0, 0, 0, b"")] and h["D_5"][0][1] == 0 and h["D_6"][0][1] == 0x0302
    assert h["M_beyond_D"][0][7] == b"cut.example" and h["M_cuts_extensions"][0][4:] == (1, 0, 0, b"")
    # (field reads are bounded by D, not M: the empty ClientHello's version is the ServerHello's first two bytes)
    assert kinds("M_4_then_hello") == [CL, SV] and h["M_4_then_hello"][0][1] == 0x0200
    assert h["sni_L0"][0][6:] == (SNI, b"") and h["sni_L1"][0][6:] == (SNI | MAL, b"") and h["sni_L1"][0][4] == 2
    assert h["sni_L4"][0][6:] == (SNI | MAL, b"") and h["sni_L5"][0][6:] == (SNI, b"")
    assert h["sni_L5_wants_more"][0][6:] == (SNI | TR, b"")
    assert h["sni_cut_by_L"][0][6:] == (SNI | TR, b"long.name.example") and h["sni_shorter_than_L"][0][6:] == (SNI, b"short")
    assert [h[n][0][7] for n in ("sni_first", "sni_middle", "sni_last", "sni_twice")] == \
        [b"first.example", b"middle.example", b"last.example", b"one.example"]
    assert h["sni_malformed_then_good"][0][6:] == (SNI | MAL, b"") and h["sni_non_ascii"][0][7] == b"n\xe4me\x00.example"
    assert h["no_extensions"][0][4:] == (0, 0, 0, b"") and h["extension_overruns"][0][4:] == (1, 0, 0, b"")
    assert h["ext_len_short"][0][4:] == (1, 0, 0, b"") and h["session_id_32"][0][5:] == (32, SNI, b"sid.example")
    assert h["session_id_beyond_D"][0][5] == 4 and h["many_ciphers"][0][3] == 90
    assert h["cipher_count_beyond_D"][0][3:5] == (16383, 0)
    assert h["v43_len0"][0][1] == 0x0303 and h["v43_len2"][0][1] == 0x0304 and h["v43_len3"][0][1] == 0x0304
    assert h["v43_len3_other"][0][1] == 0x0303 and h["v43_len4"][0][1] == 0x0303 and h["v43_twice"][0][1] == 0x7F1C
    assert h["v43_behind_others"][0][1] == 0x0304 and h["v43_in_client"][0][1] == 0x0303
    assert h["sni_in_server"][0][6:] == (HC, b"") and h["server_no_extensions"][0][2:5] == (0xC02F, 0, 0)
    assert h["cipher_cut_D40"][0][2] == 0 and h["cipher_cut_D40"][0][6] == 0 and h["cipher_cut_D41"][0][6] == HC
    assert h["cipher_behind_sid"][0][2:] == (0xC02F, 0, 0, 8, HC, b"") and h["cipher_cut_behind_sid"][0][5:7] == (8, 0)
    assert h["server_D39"][0][5:7] == (0, 0)
    # the later entries: the record's `layer` names the entry
    le = sc.run_reference(BY_NAME["later_entries"])
    lay = [[int(r["layer"]) for r in le.records() if int(r["msg"]) == j] for j in range(5)]
    assert lay == [[4], [5], [5], [3, 4, 5, 5], [5]]
    assert [int(r["kind"]) for r in le.records() if int(r["msg"]) == 3] == [CL, SV, CL, SV]
    off = [int(r["msg_offset"]) for r in le.records() if int(r["msg"]) == 3]
    assert off == sorted(off) and len(set(off)) == 4
    mr = sc.run_reference(BY_NAME["many_records"]).messages()
    assert [int(x["n_handshake"]) + int(x["n_appdata"]) for x in mr] == list(range(1, 14))
    assert [int(x) for x in mr["n_hellos"]] == [1] + [2] * 12
    # every disposition is reached; rule 2 over all flag combinations, and the flags win over recorded entries
    seen = set()
    for c in CASES:
        if c.want_disp and c.name not in sc.OVERFLOWING:
            seen |= set(_disp(c.name))
    assert seen == {sc.NONE, sc.MSG, sc.HOST, sc.BAD}
    fl = _disp("flags")
    for k, f in enumerate(sc.flag_combinations()):
        assert fl[k] == (sc.HOST if sl.incomplete_chain(f, 4, sc.ML) else sc.NONE), hex(f)
    assert fl[:256].count(sc.NONE) == 10
    M, N, H = sc.MSG, sc.NONE, sc.HOST
    assert fl[256:] == [M] * 6 + [H, H, H, H, M, H]
    r = _disp("records")
    assert r == [M, M, M, M, N, N, M, M, M, M, M, M, M, M, M, M, N, H, N, M]
    rm = sc.run_reference(BY_NAME["records"]).messages()
    rec = dict(zip([k for k, d in enumerate(r) if d == M], rm))
    assert int(rec[1]["layer_offset"]) == int(rec[0]["layer_offset"]) + 5 + len(sc.CH) and int(rec[1]["n_hellos"]) == 0
    assert int(rec[3]["n_handshake"]) == 0 and int(rec[3]["n_appdata"]) == 1
    assert mix(rec[6]) == (0, 0, 0, 0, 0) and mix(rec[7]) == (1, 0, 0, 0, 0) and int(rec[8]["n_hellos"]) == 1
    for k in (9, 10, 11, 13):
        assert int(rec[k]["flags"]) == abi.SSL_NO_TCP and int(rec[k]["src_port"]) == int(rec[k]["ssl_port"]) == 0, k
    assert int(rec[12]["flags"]) == 0 and mix(rec[14]) == (1, 0, 0, 1, 1) and mix(rec[15]) == (1, 0, 0, 0, 1)
    assert mix(rec[19]) == (1, 0, 0, 0, 1)  # the record of type 24 counts nowhere
    assert set(_disp("max_layers_1")) == {H} and set(_disp("max_layers_3")) == {H} and set(_disp("max_layers_16")) == {M}
    pm = sc.run_reference(BY_NAME["ports"]).messages()
    # (neither port an SSL port: the destination's, which for the server's packet is the client's port 40002)
    assert [int(x) for x in pm["ssl_port"]] == [443, 993, 261, 995, 8443, 80, 443, 465, 40002, 993]
    d = _disp("descriptors")
    assert [d[i] for i in (5, 11, 17, 22, 30)] == [sc.BAD] * 4 + [N]
    assert int(BY_NAME["descriptors"].offsets.max()) > 1 << 63  # the 64-bit wrap
    # the parse's own records find every packet, the crafted ones too
    pmx = abi.ssl_totals_dict(sc.run_reference(BY_NAME["parsed_mixed"]).totals)
    assert pmx["msgs"] >= 270 and pmx["host_n"] == 0
    assert abi.ssl_totals_dict(sc.run_reference(BY_NAME["parsed_ml3"]).totals)["host_n"] == 64
    # batch shapes: SSL packets at both edges of each block
    for n in sc.SIZES:
        t = abi.ssl_totals_dict(sc.run_reference(BY_NAME[f"n{n}_s1"]).totals)
        plain = len([k for k in range(0, n, 97)])
        assert plain <= t["msgs"] <= plain + sc.heavy_count(n) and t["hellos"] >= 3 * sc.heavy_count(n)
        assert abi.ssl_totals_dict(sc.run_reference(BY_NAME[f"n{n}_s100"]).totals)["msgs"] == n
    disp = _disp("n2049_s1")
    assert [disp[i] for i in (0, 1023, 1024, 2047, 2048)] == [M] * 5
    # kinds choose the hello records, never the messages' own values
    full = sc.run_reference(BY_NAME["kinds_3"])
    for kinds_ in range(4):
        got = sc.run_reference(BY_NAME[f"kinds_{kinds_}"])
        for f in ("index", "layer_offset", "payload_len", "ssl_port", "n_handshake", "n_ccs", "n_alert", "n_appdata"):
            assert (got.messages()[f] == full.messages()[f]).all(), (kinds_, f)
        keep = full.records()[[bool((kinds_ >> (int(x) - 1)) & 1) for x in full.records()["kind"]]]
        for f in ("msg", "msg_offset", "name_len", "version", "cipher", "n_ext", "kind", "layer", "flags"):
            assert (got.records()[f] == keep[f]).all(), (kinds_, f)
    # capacities: the totals hold the full would-be values under every overflow
    m_, k_, nb = sc.needs(BY_NAME["cap_exact"])
    for name in ("cap_exact", "cap_spec_exact", "cap_no_names", "cap_roomy") + sc.OVERFLOWING:
        t = abi.ssl_totals_dict(sc.run_reference(BY_NAME[name]).totals)
        assert (t["msgs"], t["hellos"], t["name_bytes"], t["overflow"]) == (m_, k_, nb, int(name in sc.OVERFLOWING)), name
    no_names, with_names = sc.run_reference(BY_NAME["cap_no_names"]), sc.run_reference(BY_NAME["cap_exact"])
    assert (no_names.records(k_) == with_names.records(k_)).all()  # positions and lengths without the names
    assert (no_names.messages(m_) == with_names.messages(m_)).all()


# ---------------------------------------------------------------- CPU: the reference's own vectors
def capture_case(b: PacketBatch, name: str, opts=None, **kw) -> sc.Case:
    """A capture through the parse's restatement: the records the device parse writes."""
    opts = opts or abi.make_opts()
    summary, layers = oracle.oracle_parse(b, opts)
    return sc.Case(name, np.concatenate([b.data, np.zeros(1, np.uint8)]), b.offsets, b.caplens, summary,
                   np.ascontiguousarray(layers).reshape(b.n, opts.max_layers), ml=opts.max_layers,
                   data_len=int(b.caplens.sum()), **kw)


_GOLDEN: dict = {}
GOLDEN_FILES = sorted(str(f) for f in np.load(VECTORS / "expected.npz", allow_pickle=False)["files"])


def frozen() -> dict:
    if "frozen" not in _GOLDEN:
        z = np.load(VECTORS / "expected.npz", allow_pickle=False)  # tools/make_golden_ssl.py
        _GOLDEN["frozen"] = {str(f): json.loads(z[f"f{k}"].tobytes().decode()) for k, f in enumerate(z["files"])}
    return _GOLDEN["frozen"]


def golden_batch(name: str) -> PacketBatch:
    if name not in _GOLDEN:
        _GOLDEN[name] = read_pcap(VECTORS / name)
    return _GOLDEN[name]


def golden_case(name: str) -> sc.Case:
    if ("case", name) not in _GOLDEN:
        _GOLDEN[("case", name)] = capture_case(golden_batch(name), name)
    return _GOLDEN[("case", name)]


def frozen_rows(msgs, hellos, names, layers, n_layers) -> dict:
    """A call's records in the shape of expected.npz's entries, per source packet with a message. layers / n_layers:
    the records the call read: an SSL layer of the reference is a followed entry here, in order."""
    names = bytes(names)
    per = {}
    for j, m in enumerate(msgs):
        i = int(m["index"])
        entries = [k for k in range(int(n_layers[i])) if int(layers[i][k]["proto"]) == sl.P_SSL]
        lay = {k: [None, None, None] for k in entries}
        for h in hellos[int(m["first_hello"]):int(m["first_hello"]) + int(m["n_hellos"])]:
            assert int(h["msg"]) == j
            fl, pos = int(h["flags"]), int(h["name_pos"])
            if int(h["kind"]) == abi.SSL_CLIENT:
                name = names[pos:pos + int(h["name_len"])].hex() if fl & abi.SSL_HAS_SNI else None
                row = [int(h["version"]), int(h["session_id_len"]), int(h["n_ciphers"]), 1, int(h["n_ext"]), name, fl]
            else:
                row = [int(h["version"]), int(h["session_id_len"]), int(h["cipher"]), (fl >> 3) & 1, int(h["n_ext"]),
                       None, fl]
            lay[int(h["layer"])][int(h["kind"])] = row
        per[i] = [int(m["payload_len"]), int(m["src_port"]), int(m["dst_port"]),
                  tuple(int(m[f]) for f in ("n_ccs", "n_alert", "n_handshake", "n_appdata")), [lay[k] for k in entries]]
    return per


def assert_frozen(per: dict, name: str) -> int:
    """Exactly the packets the real reference builds an SSL layer in, and what it reports of each; a hello marked
    undefined is compared in what is defined of it. Returns the number of hellos compared."""
    want = frozen()[name]
    assert len(want) == golden_batch(name).n
    compared = 0
    for i, w in enumerate(want):
        g = per.get(i)
        assert (g is None) == (w is None), (name, i)
        if w is None:
            continue
        assert g[:3] == w[:3], (name, i, g[:3], w[:3])
        assert g[3] == tuple(sum(1 for x in w[3] if x[0] == t) for t in (20, 21, 22, 23)), (name, i)
        assert len(g[4]) == len(w[3]), (name, i)
        for k, (gl, wl) in enumerate(zip(g[4], w[3])):
            for kind in (1, 2):
                gh, wh = gl[kind], wl[kind]
                assert (gh is None) == (wh is None), (name, i, k, kind)
                if wh is None:
                    continue
                compared += 1
                if wh[6]:  # undefined in the reference: the departure of rule 6 / rule 7
                    assert gh[1:5] == wh[1:5] and gh[5] in (None, ""), (name, i, k, gh, wh)
                    if kind == 1:
                        assert gh[0] == wh[0] and gh[6] & abi.SSL_SNI_MALFORMED
                    continue
                assert gh[:6] == wh[:6], (name, i, k, gh, wh)
    return compared


@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_reference_reproduces_the_real_ssl_layers(name):
    """No packet is left out: a packet has a message exactly where the reference builds an SSL layer behind TCP, and
    every hello of every handshake layer is the reference's; the marked undefined hellos equal the model."""
    c = golden_case(name)
    got = sc.run_reference(c)
    t = abi.ssl_totals_dict(got.totals)
    assert t["host_n"] == 0 and t["overflow"] == 0 and t["bad_desc"] == 0
    compared = assert_frozen(frozen_rows(got.messages(), got.records(), got.name_bytes(), c.layers,
                                         c.summary["n_layers"]), name)
    assert compared == t["hellos"]
    sc.assert_same(got, sc.model(c), name)


def test_golden_data_holds_the_oddities():
    """What the crafted set is there for, read off the real layers' frozen answers."""
    crafted = [p for p in frozen()["crafted.pcap"] if p is not None]
    hellos = [(kind, h) for p in crafted for lay in p[3] for kind, h in ((1, lay[1]), (2, lay[2])) if h is not None]
    assert len(frozen()["crafted.pcap"]) >= 2200 and len(crafted) >= 2000 and len(hellos) >= 1500
    assert sum(1 for _, h in hellos if h[6]) >= 10                                 # undefined in the reference
    assert sum(1 for k, h in hellos if k == 1 and h[5] == "") >= 3                 # an empty name that counts
    assert sum(1 for k, h in hellos if k == 1 and h[5] is None and not h[6]) >= 50  # no SNI
    assert sum(1 for k, h in hellos if k == 2 and not h[3]) >= 3                   # the cipher word cut
    assert sum(1 for p in crafted if all(lay[1] is None and lay[2] is None for lay in p[3])) >= 100
    assert sum(1 for p in crafted for lay in p[3] if lay[1] and lay[2]) >= 3       # both hellos in one layer
    assert max(len(p[3]) for p in crafted) == 13
    assert frozen()["packet_examples.pcap"].count(None) == 0


def report_tables(path: Path) -> dict:
    """The numbers and table rows of an SSLAnalyzer report, but the sample-time and rate lines."""
    out = {"ports": {}, "versions": {}, "ciphers": {}, "hosts": {}}
    keys = {"Number of SSL packets": "packets", "Number of SSL flows": "flows", "Total SSL data": "data",
            "Average packets per flow": "packets_per_flow", "Average data per flow": "data_per_flow",
            "Client-hello message": "client_hellos", "Server-hello message": "server_hellos",
            "Number of SSL flows with successful handshake": "handshake_complete",
            "Number of SSL flows ended with alert": "alerts"}
    tables = {"SSL/TLS ports": "ports", "SSL/TLS version": "versions", "Cipher-suite": "ciphers", "Hostname": "hosts"}
    table = None
    for line in path.read_text().split("\n"):
        m = re.match(r"^([^:|]+):\s+([0-9.]+) \[", line)
        if m and m.group(1) in keys:
            out[keys[m.group(1)]] = float(m.group(2)) if "." in m.group(2) else int(m.group(2))
        m = re.match(r"^\| (.*?)\s*\| (\S+)\s*\|$", line)
        if m and m.group(2) == "Count":
            table = tables[m.group(1)]
        elif m:
            key = {"ports": int, "versions": VERSIONS.get, "ciphers": IANA_SUITES.get, "hosts": str}[table](m.group(1))
            assert key is not None, line
            out[table][key] = int(m.group(2))
    return out


def assert_report(tables: dict, name: str) -> None:
    want = report_tables(VECTORS / REPORTS[name])
    assert len(want) == 13 and all(want[t] for t in ("ports", "versions", "ciphers", "hosts"))
    got = dict(tables)
    for f in ("packets_per_flow", "data_per_flow"):  # printed with three decimals
        assert f"{got.pop(f):.3f}" == f"{want.pop(f):.3f}", f
    assert got == want


@pytest.mark.parametrize("name", sorted(REPORTS))
def test_analyze_reproduces_the_ssl_analyzers_reports(name):
    c = golden_case(name)
    got = sc.run_reference(c)
    assert_report(sl.analyze(got.messages(), got.records(), got.name_bytes(), c.summary["hash5"]), name)
    t = abi.ssl_totals_dict(got.totals)
    assert t["msgs"] == {"tls.pcap": 17, "many_protocols_ssl.pcap": 401}[name]


def _case_file(c: sc.Case, path: Path) -> None:
    want = sc.model(c)
    rec = sc.brief_of(c)[:c.n] if c.use_brief else c.summary
    spec = np.frombuffer(bytes(sc.spec_of(c)), np.uint8)
    head = np.array([c.n, c.dlen(), c.ml, 0 if c.use_brief else 1, c.maxm(), c.maxh(), c.cap(), int(c.want_names),
                     int(c.want_disp)], np.uint64)
    parts = [head, spec, c.data[:c.dlen()], c.offsets, c.caplens, rec, c.layers, want.msgs[:c.maxm() * 32],
             want.hellos[:c.maxh() * 32]]
    parts += [want.names[:c.cap()]] if c.want_names else []
    parts += [want.disposition[:c.n]] if c.want_disp else []
    parts.append(want.totals)
    path.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))


def test_reference_under_sanitizers(tmp_path):
    """pcppx_ssl_reference in a stand-alone program (its own main, host compiler, no HIP, nothing loaded into python)
    built with ASan + UBSan: the case families in exact-size heap buffers, the results equal to the model's."""
    gxx = shutil.which("g++")
    assert gxx is not None
    exe = tmp_path / "ssl_ref_check"
    csrc = abi.PKG_DIR / "csrc"
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(HEADER.parent), "-I", str(csrc),
                    str(abi.REPO_DIR / "tests" / "native" / "ssl_ref_check.cpp"),
                    str(csrc / "pcppx_ssl_ref.cpp"), "-o", str(exe)], check=True)
    files = []
    for name in ("record_types", "hellos", "later_entries", "many_records", "fuzz", "fuzz_server", "flags", "records",
                 "max_layers_4", "ports", "descriptors", "parsed_mixed", "n65_s100", "n1025_s1", "n0", "n65_brief",
                 "kinds_0", "kinds_1", "kinds_2", "cap_exact", "cap_msgs_short1", "cap_hellos_short1",
                 "cap_names_short1", "cap_spec_short1", "cap_no_names", "cap_sizing"):
        path = tmp_path / f"{name}.case"
        _case_file(BY_NAME[name], path)
        files.append(str(path))
    path = tmp_path / "crafted.case"  # the mutated real hellos too
    _case_file(golden_case("crafted.pcap"), path)
    files.append(str(path))
    env = {"TMPDIR": str(tmp_path), "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count(" ok\n") == len(files)


TOOL = [sys.executable, str(abi.REPO_DIR / "tools" / "ssl_file.py")]


def test_ssl_file_tool_without_gpu(tmp_path):
    """tools/ssl_file.py --reference: SSLAnalyzer's tables and the rows of a golden capture, without a GPU."""
    name = "tls.pcap"
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "--analyze"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    tables = json.loads(run.stdout)
    assert_report({k: {int(x) if k != "hosts" else x: n for x, n in v.items()} if isinstance(v, dict) else v
                   for k, v in tables.items()}, name)
    out = tmp_path / "rows.txt"
    run = subprocess.run(TOOL + ["-r", str(VECTORS / name), "--reference", "-o", str(out)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert out.read_text().split("\n") == [sl.format_row(r) for r in sc.run_reference(golden_case(name)).rows()] + [""]
    assert out.read_text().count("\n") == 6


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_ssl_equals_reference(engine, case):
    """Whole buffers, 0xA5 guards included: records, names, dispositions and totals, and nothing outside them."""
    want = sc.run_reference(case)
    got = sc.run_device(engine, case)
    sc.assert_same(got, want, case.name)
    if case.name in sc.OVERFLOWING:
        sc.assert_untouched(got, case.name)


@pytest.mark.gpu
def test_gpu_ssl_sizing_then_exact(engine):
    """The sizing call (no room at all) gives the three sizes; the call with exactly that room succeeds."""
    base = BY_NAME["cap_exact"]
    t = abi.ssl_totals_dict(sc.run_device(engine, BY_NAME["cap_sizing"]).totals)
    assert t["overflow"] == 1
    exact = replace(base, out_msgs=t["msgs"], out_hellos=t["hellos"], names_cap=t["name_bytes"])
    got = sc.run_device(engine, exact)
    assert int(got.totals[abi.SSL_OVERFLOW]) == 0
    sc.assert_same(got, sc.run_reference(exact), "exact")
    no_names = sc.run_device(engine, BY_NAME["cap_no_names"])
    assert (no_names.records(t["hellos"]) == got.records(t["hellos"])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n1025_s100", "n2049_s1", "kinds_2", "cap_names_short1", "cap_no_names"])
def test_gpu_ssl_is_repeatable_across_streams(engine, name):
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
def test_gpu_ssl_source_on_both_sides_of_4gib(engine):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32
    (the layout of test_http.py's case): one SSL packet lies across each line."""
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
    want = sc.run_reference(compact)
    assert int(want.totals[abi.SSL_MSGS]) == n
    assert {bool(o < wc.LINE) for o in wide.offsets} == {True, False}
    got = sc.run_device(engine, compact, source=source)
    sc.assert_same(got, want, "wide")
    del raw, data, source
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_FILES)
def test_gpu_golden_captures_from_a_device_parse(engine, name):
    """Parsed on the device, walked on the device: what the real SSL layers report, and for the two captures of the
    reference's SSLAnalyzer test the report it expects."""
    from pcapplusplus_amd.engine import ssl_on_device

    b = golden_batch(name)
    msgs, hellos, names, hash5, disp, tot = ssl_on_device(engine, b)
    assert tot["host_n"] == 0 and tot["msgs"] == len(msgs) == int((disp == abi.SSL_MSG).sum())
    c = golden_case(name)
    assert_frozen(frozen_rows(msgs, hellos, names, c.layers, c.summary["n_layers"]), name)
    if name in REPORTS:
        assert_report(sl.analyze(msgs, hellos, names, hash5), name)
