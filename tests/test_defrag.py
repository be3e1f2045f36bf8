"""pcppx_defrag_device: the IPv4 fragment groups that are complete inside one device batch (include/pcppx.h, defrag).

CPU: the ctypes mirrors match the header and every bad-argument combination is refused before any device work;
pcppx_defrag_reference (the contract in plain C++ over host pointers) equals a brute-force Python restatement of the
contract on every case family of tests/defrag_cases.py, byte for byte, the 0xA5 fill of everything else included (all of
it but the totals on overflow); a second model, IPReassembly::processPacket restated as a streaming machine, reproduces
the reference's own test vectors (tests/golden/defrag: data files of Tests/Pcap++Test/PcapExamples), and every packet
the contract reassembles, in any order of arrival, is the packet that machine returns at the same source position.
GPU: pcppx_defrag_device equals pcppx_defrag_reference byte for byte on the same cases; two calls on two streams agree
and a repeat is bit-identical; source packets on both sides of offset 2^32; fragment -> parse + reasm -> defrag -> parse
gives the records, the hash5 and the filter verdicts of the unfragmented batch; the reference's vectors on the device.
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

import defrag_cases as dc
import oracle
from conftest import GOLDEN
from pcapplusplus_amd import abi, frag
from pcapplusplus_amd.pcap import PacketBatch, from_packets, read_hex_dat, read_pcap

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
VECTORS = GOLDEN / "defrag"
CASES = dc.cases()
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if c.n <= 3200]


# ---------------------------------------------------------------- CPU: the ABI
def test_defrag_structs_match_header():
    fields = {"pcppx_defrag_spec": abi.DefragSpec, "pcppx_defragged": abi.Defragged}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    consts = ["PCPPX_DEFRAG_MAX_FRAGS", "PCPPX_DEFRAG_PASS", "PCPPX_DEFRAG_LEFT", "PCPPX_DEFRAG_MERGED",
              "PCPPX_DEFRAG_MERGED_LAST", "PCPPX_DEFRAG_BAD_DESC", "PCPPX_DEFRAG_OUT_PACKETS", "PCPPX_DEFRAG_OUT_BYTES",
              "PCPPX_DEFRAG_REASSEMBLED", "PCPPX_DEFRAG_MERGED_FRAGS", "PCPPX_DEFRAG_LEFT_FRAGS",
              "PCPPX_DEFRAG_CANDIDATES", "PCPPX_DEFRAG_BAD_DESC_N", "PCPPX_DEFRAG_OVERFLOW", "PCPPX_DEFRAG_TOTALS",
              "PCPPX_ABI_VERSION"]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu\\n", sizeof(pcppx_defrag_spec), sizeof(pcppx_defragged));\n'
           '  printf("' + " ".join(["%d"] * len(consts)) + '\\n", ' + ", ".join(consts) + ");\n" + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.DefragSpec), C.sizeof(abi.Defragged)]
    assert [int(x) for x in out[1].split()] == [
        abi.DEFRAG_MAX_FRAGS, abi.DEFRAG_PASS, abi.DEFRAG_LEFT, abi.DEFRAG_MERGED, abi.DEFRAG_MERGED_LAST,
        abi.DEFRAG_BAD_DESC, abi.DEFRAG_OUT_PACKETS, abi.DEFRAG_OUT_BYTES, abi.DEFRAG_REASSEMBLED,
        abi.DEFRAG_MERGED_FRAGS, abi.DEFRAG_LEFT_FRAGS, abi.DEFRAG_CANDIDATES, abi.DEFRAG_BAD_DESC_N,
        abi.DEFRAG_OVERFLOW, abi.DEFRAG_TOTALS, abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        seen += 1
    assert seen == len(abi.DefragSpec._fields_) + len(abi.Defragged._fields_)
    assert abi.ABI_VERSION == 7 and len(abi.DEFRAG_FIELDS) == abi.DEFRAG_TOTALS


def test_defrag_symbols_are_exported():
    lib = abi.load_engine()
    for name in ("pcppx_defrag_device", "pcppx_defrag_reference"):
        assert name in abi.EXPORTED_SYMBOLS and getattr(lib, name) is not None
        assert re.search(rf"PCPPX_API int {name}\(", HEADER.read_text())


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    r = abi.Records(1, 1)
    s = abi.make_defrag_spec(True, 0)
    o = abi.Defragged(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    return dict(b=b, r=r, ml=6, info=1, s=s, o=o)


def _set(a, which, field, value):
    setattr(a[which], field, value)


def _spec_reserved(a, k):
    a["s"].reserved[k] = 1


BAD_ARGS = {
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
    "max_layers_255": lambda a: a.update(ml=255),
    "passthrough_2": lambda a: _set(a, "s", "passthrough", 2),
    "spec_reserved_0": lambda a: _spec_reserved(a, 0),
    "spec_reserved_2": lambda a: _spec_reserved(a, 2),
    "out_reserved": lambda a: _set(a, "o", "reserved", 1),
}


def _call(lib, a, ctx=C.c_void_p(1), **null):
    """(pcppx_defrag_device's, pcppx_defrag_reference's) return codes; the reference only with a bad argument."""
    ref = lambda k: None if null.get(k) else C.byref(a[k])  # noqa: E731
    dev = lib.pcppx_defrag_device(ctx, ref("b"), ref("r"), a["ml"], a["info"], ref("s"), ref("o"), None)
    host = None if ctx is None else \
        lib.pcppx_defrag_reference(ref("b"), ref("r"), a["ml"], a["info"], ref("s"), ref("o"))
    return dev, host


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_defrag_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    a = _good_args()
    BAD_ARGS[what](a)
    assert _call(abi.load_engine(), a) == (abi.E_INVAL, abi.E_INVAL)


def test_defrag_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    a = _good_args()
    assert _call(lib, a, ctx=None)[0] == abi.E_INVAL
    for k in ("b", "r", "s", "o"):
        assert _call(lib, a, **{k: True}) == (abi.E_INVAL, abi.E_INVAL), k
    # a brief instead of the summary, the optional columns absent and an empty batch without info pass the checks
    for name in ("many_groups_brief", "no_columns", "n0"):
        assert int(dc.run_reference(BY_NAME[name]).totals[abi.DEFRAG_OVERFLOW]) == 0
    empty = dc.run_reference(BY_NAME["n0"])
    assert list(empty.totals) == [0] * abi.DEFRAG_TOTALS
    dc.assert_untouched(empty, "n0")


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    got = dc.run_reference(case)
    dc.assert_same(got, dc.brute(case), case.name)
    if case.name in dc.OVERFLOWING:
        assert int(got.totals[abi.DEFRAG_OVERFLOW]) == 1
        dc.assert_untouched(got, case.name)


def _fragment_rows(c):
    st = c.info["ip_status"]
    return (st & 15 == abi.IPR_FRAGMENT) & (st & abi.IPR_F_IPV6 == 0)


def test_cases_cover_the_kernel_shapes():
    """The block size the cases are built around is the kernels', and the families reach the paths they name."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kDefragBlockPk\s*=\s*(\d+)", txt).group(1)) == dc.BLOCK
    assert int(re.search(r"PCPPX_DEFRAG_MAX_FRAGS\s+(\d+)", HEADER.read_text()).group(1)) == dc.MAX_FRAGS == 64
    assert max(c.n for c in CASES) <= 70_000 and BY_NAME["big"].n > 64 * dc.BLOCK
    for name in dc.CLEAN:  # every IPv4 fragment with an IPv4 layer is merged: nothing passes by being LEFT
        c = BY_NAME[name]
        t = abi.defrag_totals_dict(dc.brute(c).totals)
        assert t["reassembled"] >= 1 and t["merged_frags"] == t["candidates"], (name, t)
    for name in dc.UNCLEAN:
        c = BY_NAME[name]
        t = abi.defrag_totals_dict(dc.brute(c).totals)
        assert t["left_frags"] >= 1 and t["left_frags"] + t["merged_frags"] == int(_fragment_rows(c).sum()), (name, t)
    sizes = {int(f) for c in CASES if c.want_columns for f in dc.brute(c).frags[:c.n] if f not in (0, dc.FILL8)}
    assert {2, 3, 63, 64} <= sizes and max(sizes) == 64
    for n in (dc.BLOCK - 1, dc.BLOCK, dc.BLOCK + 1):  # the members of a group in two blocks
        c = BY_NAME[f"blocks_n{n}"]
        rows = _fragment_rows(c)
        for key in np.unique(c.info["ip_key"][rows]):
            members = np.nonzero(rows & (c.info["ip_key"] == key))[0]
            assert len({int(j) // dc.BLOCK for j in members}) == 2 and len({int(j) // 64 for j in members}) >= 3
    got = dc.brute(BY_NAME["blocks_first_last"])
    assert sorted((i, f) for i, f, _ in dc.reassembled(got)) == [(dc.BLOCK, dc.BLOCK), (2 * dc.BLOCK + 3, 2 * dc.BLOCK + 3)]
    op, ob, nc = dc.output_totals(BY_NAME["index_only"])
    exact = abi.defrag_totals_dict(dc.brute(BY_NAME["cap_exact"]).totals)
    assert (exact["out_packets"], exact["out_bytes"], exact["candidates"], exact["overflow"]) == (op, ob, nc, 0)
    for name in dc.OVERFLOWING:
        assert int(dc.brute(BY_NAME[name]).totals[abi.DEFRAG_OVERFLOW]) == 1, name
    for name in ("index_only", "index_only_cap_ignored", "no_columns", "only_reassembled_exact"):
        assert int(dc.brute(BY_NAME[name]).totals[abi.DEFRAG_OVERFLOW]) == 0, name
    t = abi.defrag_totals_dict(dc.brute(BY_NAME["bad_desc_pt1"]).totals)
    assert t["bad_desc"] > 20 and t["reassembled"] > 5 and t["left_frags"] > 0
    t = abi.defrag_totals_dict(dc.brute(BY_NAME["mixed"]).totals)
    assert t["left_frags"] == 2  # the two IPv6 fragments
    k = BY_NAME["keys_congruent"].info["ip_key"][_fragment_rows(BY_NAME["keys_congruent"])]
    assert 0 in k and len({int(x) % 1024 for x in k if x}) == 1
    for name in ("trailer", "df_first_last"):  # the first fragment's trailer is dropped
        c = BY_NAME[name]
        (i, f, pkt), = dc.reassembled(dc.brute(c))
        assert int(c.summary["flags"][f]) & abi.F_TRAILER and len(pkt) < sum(
            int(c.caplens[j]) for j in np.nonzero(_fragment_rows(c))[0]) - 2 * 14
    (_, _, pkt), = dc.reassembled(dc.brute(BY_NAME["gre"]))
    assert pkt[14 + 9] == 47 and pkt[14 + 6:14 + 8] == b"\0\0"  # the outer header is the one patched


# ---------------------------------------------------------------- CPU: the streaming model against the reference's data
def parsed_case(batch: PacketBatch, name: str, **kw) -> dc.Case:
    summary, layers = oracle.oracle_parse(batch, dc.OPTS)
    info = oracle.oracle_reasm(batch, summary, layers)
    return dc.Case(name, batch.data[:int(batch.caplens.sum())], batch.offsets, batch.caplens, summary=summary,
                   layers=layers, info=info, **kw)


def vector_case(name: str, **kw) -> dc.Case:
    path = VECTORS / name
    if not path.exists():  # frag_http_req.pcap came with the ingest fixtures
        path = GOLDEN / "ingest" / "files" / f"Tests__Pcap++Test__PcapExamples__{name}"
    return parsed_case(read_pcap(path), name, **kw)


def test_stream_model_reproduces_the_reference_vectors():
    """The positions are those of the reference's tests (Tests/Pcap++Test/Tests/IPFragmentationTests.cpp): the HTTP
    request on its last fragment; packets 1, 4 and 6 of ip4_fragments.pcap on the sixth (packet 1) and tenth fragment of
    theirs (TestIPFragMultipleFrags: the duplicated fragment behind packets 4 and 6 returns nothing); the padded VLAN
    datagram on its first fragment, which arrives last."""
    c = vector_case("frag_http_req.pcap")
    got = dc.stream(c)
    assert list(got) == [c.n - 1] and got[c.n - 1][0] == read_hex_dat(VECTORS / "frag_http_req_reassembled.txt")
    c = vector_case("ip4_fragments.pcap")
    got = dc.stream(c)
    assert c.n == 53 and sorted(got) == [5, 11, 17, 27, 39, 52]
    for at, name in ((5, "packet1"), (27, "packet4"), (39, "packet6")):
        assert got[at][0] == read_hex_dat(VECTORS / f"ip4_fragments_{name}.txt"), name
    c = vector_case("frag_with_padding.pcap")
    got = dc.stream(c)
    assert c.n == 8 and list(got) == [7] and got[7][1] == 7
    assert got[7][0] == read_hex_dat(VECTORS / "frag_with_padding_defragmented.dat")
    # any order of arrival gives the same HTTP request, on the last arrival
    c = vector_case("frag_http_req.pcap")
    want = read_hex_dat(VECTORS / "frag_http_req_reassembled.txt")
    for seed in range(5):
        order = np.random.default_rng(seed).permutation(c.n).tolist()
        got = dc.stream(c, order)
        assert list(got) == [c.n - 1] and got[c.n - 1][0] == want


def test_reference_on_the_vectors():
    c = vector_case("frag_http_req.pcap", passthrough=False)
    got = dc.run_reference(c)
    (i, f, pkt), = dc.reassembled(got)
    assert (i, f, pkt) == (c.n - 1, 0, read_hex_dat(VECTORS / "frag_http_req_reassembled.txt"))
    assert int(got.totals[abi.DEFRAG_OUT_PACKETS]) == 1 and int(got.frags[0]) == c.n
    c = vector_case("ip4_fragments.pcap")
    got = dc.run_reference(c)
    packets = dc.reassembled(got)
    assert [(i, f) for i, f, _ in packets] == [(5, 0), (11, 6), (17, 12)]
    assert packets[0][2] == read_hex_dat(VECTORS / "ip4_fragments_packet1.txt")
    d = got.disposition[:c.n]
    ids = c.info["frag_id"]
    assert sorted(set(ids[d == abi.DEFRAG_LEFT].tolist())) == [0x1EA3, 0x1EA4, 0x1EA5]
    assert int((d == abi.DEFRAG_LEFT).sum()) == 32 and int((d == abi.DEFRAG_PASS).sum()) == 3
    assert int((d == abi.DEFRAG_MERGED).sum()) == 15 and int((d == abi.DEFRAG_MERGED_LAST).sum()) == 3
    st = dc.stream(c)  # what the device reassembles is what the reference returns there
    for i, f, pkt in packets:
        assert st[i] == (pkt, f)
    c = vector_case("frag_with_padding.pcap", passthrough=False)
    (i, f, pkt), = dc.reassembled(dc.run_reference(c))
    assert (i, f, pkt) == (7, 7, read_hex_dat(VECTORS / "frag_with_padding_defragmented.dat"))


# ---------------------------------------------------------------- CPU: soundness
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_reassembled_packets_are_what_the_stream_returns(case):
    """In source order and in five seeded permutations: every packet the contract reassembles equals, byte for byte and
    at the same position, what processPacket returns for that order of arrival; the clean families reassemble all."""
    if not case.want_columns or case.index_only or case.name in dc.OVERFLOWING:
        case = replace(case, want_columns=True, want_index=True, index_only=False, data_cap=None, max_packets=None,
                       max_fragments=0)
    orders = [np.arange(case.n)] + [np.random.default_rng(100 + s).permutation(case.n) for s in range(5)]
    for perm in orders:
        c = dc.permuted(case, perm)
        got = dc.run_reference(c)
        st = dc.stream(c)
        packets = dc.reassembled(got)
        assert len(packets) == int(got.totals[abi.DEFRAG_REASSEMBLED])
        for i, f, pkt in packets:
            assert i in st and st[i] == (pkt, f), (case.name, i)
        if case.name in dc.CLEAN:
            assert int(got.totals[abi.DEFRAG_MERGED_FRAGS]) == int(got.totals[abi.DEFRAG_CANDIDATES]) > 0
            assert sorted(st) == sorted(i for i, _, _ in packets)  # and the stream returns nothing else


# ---------------------------------------------------------------- CPU: the fragmenter
def _udp_batch(n: int, seed: int) -> PacketBatch:
    rng = np.random.default_rng(seed)
    pk = []
    for k in range(n):
        size = int(rng.choice([8, 30, 64, 65, 200, 1000, 1472]))
        l4 = dc.udp_datagram(rng, size, 1024 + k % 50, 2000 + k % 7) if k % 3 else \
            dc.struct.pack(">HHIIBBHHH", 1024 + k, 80, k, 0, 0x50, 0x10, 512, 0, 0) + bytes(rng.integers(0, 256, size - 8, dtype=np.uint8))
        pk.append(dc.eth(7 if k % 4 == 0 else None) +
                  dc.ipv4(0x0A000000 + k % 97, 0x0B000000 + k % 89, k, l4, proto=17 if k % 3 else 6, df=k % 5 == 0))
    pk[3] = dc.eth(ethertype=0x0806) + bytes(28)
    pk[5] = dc.ipv6_fragment(rng, 5)
    return from_packets(pk)


def test_fragmenter_follows_ipfragutil():
    base = _udp_batch(200, 3)
    out = frag.fragment(base, 60)  # rounded down to 56
    src, no, cnt = out.meta["frag_src"], out.meta["frag_no"], out.meta["frag_count"]
    v4, ip_off, hdr, pay = frag.locate_ipv4(base)
    assert not v4[3] and not v4[5] and v4.sum() == 198
    summary, layers = oracle.oracle_parse(out, dc.OPTS)
    info = oracle.oracle_reasm(out, summary, layers)
    for i in range(base.n):
        rows = np.nonzero(src == i)[0]
        if not v4[i] or pay[i] <= 56:
            assert len(rows) == 1 and out.packet(int(rows[0])) == base.packet(i)
            continue
        assert len(rows) == -(-int(pay[i]) // 56) == int(cnt[rows[0]]) and list(no[rows]) == list(range(len(rows)))
        p = base.packet(i)
        o, h = int(ip_off[i]), int(hdr[i])
        body = b""
        for k, r in enumerate(rows):
            q = out.packet(int(r))
            assert q[:o] == p[:o] and q[o + 12:o + h] == p[o + 12:o + h] and q[o + 8:o + 10] == p[o + 8:o + 10]
            assert dc.header_checksum(q[o:o + h]) == 0  # the checksum verifies
            assert int.from_bytes(q[o + 2:o + 4], "big") == len(q) - o
            word = int.from_bytes(q[o + 6:o + 8], "big")
            assert word == (k * 56 // 8) | (0x2000 if k + 1 < len(rows) else 0)  # DF cleared
            assert int(info["ip_status"][r]) & 15 == abi.IPR_FRAGMENT and int(info["frag_offset"][r]) == k * 56
            body += q[o + h:]
        assert body == p[o + h:o + h + int(pay[i])]
    only = frag.fragment(base, 56, select=np.arange(base.n) % 2 == 0)
    assert set(only.meta["frag_src"][only.meta["frag_count"] > 1] % 2) == {0}
    with pytest.raises(ValueError):
        frag.fragment(base, 7)


def test_fragment_then_reference_gives_the_datagrams_back():
    base = _udp_batch(300, 4)
    fr = frag.fragment(base, 576)
    c = parsed_case(fr, "round_trip")
    got = dc.run_reference(c)
    t = abi.defrag_totals_dict(got.totals)
    assert t["out_packets"] == base.n and t["left_frags"] == 1 and t["merged_frags"] == t["candidates"] > 50
    out = PacketBatch(got.data, got.offsets[:base.n], got.caplens[:base.n])
    for j in range(base.n):
        want = bytearray(base.packet(j))
        if got.frags[j]:  # DF is gone and the checksum follows: the reference's computeCalculateFields does the same
            o = 18 if want[12:14] == b"\x81\x00" else 14
            want = dc.patched(want, o, 20, len(want) - o - 20)
        assert out.packet(j) == bytes(want), j
    assert list(fr.meta["frag_src"][got.first[:base.n]]) == list(range(base.n))


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_defrag_equals_reference(engine, case):
    want = dc.run_reference(case)
    got = dc.run_device(engine, case)
    dc.assert_same(got, want, case.name)
    if case.name in dc.OVERFLOWING:
        dc.assert_untouched(got, case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["many_groups", "g64_shuffled", "big", "maxf_short1", "only_reassembled"])
def test_gpu_defrag_is_repeatable_across_streams(engine, name):
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


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 9])
def test_gpu_defrag_source_on_both_sides_of_4gib(engine, mis):
    """The packets of a small case laid around offset 2^32 and around the offset whose address is a multiple of 2^32:
    one packet lies across each line, members of one group on both sides."""
    import torch

    import wide_cases as wc

    case = BY_NAME["many_groups_brief"]
    case = replace(case, src_misalign=0, out_misalign=3)
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
    want = dc.run_reference(compact)
    assert int(want.totals[abi.DEFRAG_REASSEMBLED]) == 40
    sides = [{bool(wide.offsets[j] < wc.LINE) for j in np.nonzero(compact.info["ip_key"] == k)[0]}
             for k in np.unique(compact.info["ip_key"][_fragment_rows(compact)])]
    assert any(len(s) == 2 for s in sides)
    got = dc.run_device(engine, compact, source=source)
    dc.assert_same(got, want, f"wide mis{mis}")
    del raw, data, source
    torch.cuda.empty_cache()


def _device_parse_reasm(engine, batch: PacketBatch, opts):
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
def test_gpu_fragment_parse_defrag_parse_end_to_end(engine):
    from pcapplusplus_amd.engine import defrag_on_device, parse_on_device
    from test_filter import gpu_filter

    base = _udp_batch(1500, 6)
    fr = frag.fragment(base, 576)
    assert fr.n > base.n + 300
    summary, layers, info = _device_parse_reasm(engine, fr, dc.OPTS)
    assert int((summary["hash5"][info["frag_offset"] > 0] != 0).sum()) == 0  # what the feature is for
    out, index, first, frags, disp, tot = defrag_on_device(engine, fr, summary, layers, info, passthrough=True)
    assert tot["out_packets"] == base.n and tot["overflow"] == 0 and tot["left_frags"] == 1
    assert tot["reassembled"] == int((frags != 0).sum()) > 300 and tot["merged_frags"] == tot["candidates"]
    assert list(fr.meta["frag_src"][first]) == list(range(base.n))
    # the expected bytes: the original packets, a reassembled one with DF cleared and its checksum recomputed
    pk = []
    for j in range(base.n):
        p = bytearray(base.packet(j))
        if frags[j]:
            o = 18 if p[12:14] == b"\x81\x00" else 14
            p = dc.patched(p, o, 20, len(p) - o - 20)
        pk.append(bytes(p))
    want = from_packets(pk)
    assert [out.packet(j) for j in range(base.n)] == pk
    got_s, got_l = parse_on_device(engine, out, dc.OPTS)
    want_s, want_l = oracle.oracle_parse(want, dc.OPTS)
    oracle.compare_exact(got_s, got_l, want_s, want_l)
    base_s, _ = oracle.oracle_parse(base, dc.OPTS)
    assert (got_s["hash5"] == base_s["hash5"]).all() and (got_s["l4_layer"] == base_s["l4_layer"]).all()
    l4 = (np.arange(base.n) != 3) & (np.arange(base.n) != 5)
    assert (got_s["l4_layer"][l4] != 0xFF).all() and (got_s["hash5"][l4] != 0).all()
    for spec in (oracle.make_spec(dst_port=2003), oracle.make_spec(src_ip="10.0.0.5", protocol=5)):
        a = gpu_filter(engine, out, spec)
        b = gpu_filter(engine, base, spec)
        assert (a[0] == b[0]).all() and int(a[0].sum()) > 0


@pytest.mark.gpu
def test_gpu_defrag_on_the_reference_vectors(engine):
    from pcapplusplus_amd.engine import defrag_on_device

    for name, passthrough in (("frag_http_req.pcap", False), ("ip4_fragments.pcap", True),
                              ("frag_with_padding.pcap", False)):
        c = vector_case(name, passthrough=passthrough)
        dc.assert_same(dc.run_device(engine, c), dc.run_reference(c), name)
    b = read_pcap(VECTORS / "frag_with_padding.pcap")
    summary, layers, info = _device_parse_reasm(engine, b, dc.OPTS)
    out, index, first, frags, disp, tot = defrag_on_device(engine, b, summary, layers, info, passthrough=False)
    assert out.n == 1 and out.packet(0) == read_hex_dat(VECTORS / "frag_with_padding_defragmented.dat")
    assert (list(index), list(first), list(frags)) == ([7], [7], [8]) and out.timestamps_ns[0] == b.timestamps_ns[7]
