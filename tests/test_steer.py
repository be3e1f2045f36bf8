"""pcppx_steer_device: stable K-way flow steering of a device batch into packed sub-batches (include/pcppx.h, steer).

CPU: pcppx_steer_reference (the contract in plain C++ over host pointers) equals a brute-force per-packet Python loop
on every case family of tests/steer_cases.py; the ctypes mirrors match the header; every bad-argument combination is
refused before any device work; a crafted stream shows that contiguous sharding changes FilterTraffic's verdicts and
that steering by hash5 does not.
GPU: pcppx_steer_device equals pcppx_steer_reference byte for byte -- data, offsets, caplens, index, bucket_first,
bucket_pos, totals, and the 0xA5 fill of everything else (all of it on overflow) -- on the same cases; two calls on two
streams agree; over a real parse the key may be read through the summary, the brief, the tuples or the flow_keys
column; every bucket is an ordinary batch (closure under parse); per-bucket filtering with separate flow tables equals
the single worker's verdicts; and steer -> D2H -> write_pcap writes every packet exactly once, in capture order.
"""
from __future__ import annotations

import ctypes as C
import re
import struct
import subprocess
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import oracle
import steer_cases as tc
from conftest import golden_files, load_golden
from pcapplusplus_amd import abi
from pcapplusplus_amd.pcap import PacketBatch, from_packets
from test_filter import OPTS as FILTER_OPTS
from test_filter import gpu_filter

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
CASES = tc.cases()
BY_NAME = {c.name: c for c in CASES}
OVERFLOWING = ("cap_short1", "cap_half", "cap_zero", "maxp_short1", "maxp_zero", "cap_zero_maxp_zero",
               "index_only_maxp_short1", "no_index_overflow")


# ---------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_brute_force(case):
    got = tc.run_reference(case)
    tc.assert_same(got, tc.brute(case), case.name)
    if case.name in OVERFLOWING:
        assert int(got.totals[abi.STEER_OVERFLOW]) == 1
        tc.assert_untouched(got, case.name)


def test_cases_cover_the_kernel_shapes():
    """The block size and the scan step the cases are built around are the kernels', and the families reach the paths
    they name."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_internal.h").read_text()
    assert int(re.search(r"kSteerBlockPk\s*=\s*(\d+)", txt).group(1)) == tc.BLOCK
    assert int(re.search(r"kSteerScanStep\s*=\s*(\d+)", txt).group(1)) == tc.SCAN_STEP
    assert max(c.n for c in CASES if not c.name.startswith("scan3")) <= 100_000
    blocks = lambda c: -(-c.n // tc.BLOCK)  # noqa: E731
    s3 = BY_NAME["scan3_k2_drops_bad"]  # more than two steps of the dropped / bad sums, with something to sum in each
    assert s3.n_buckets == 2 and blocks(s3) > 2 * 256 > 2 * tc.SCAN_STEP and int(s3.caplens.max()) <= 8
    t = tc.brute(s3).totals
    assert int(t[abi.STEER_DROPPED]) > blocks(s3) and int(t[abi.STEER_BAD_DESC]) > blocks(s3) // 4
    for lo in range(0, s3.n, tc.SCAN_STEP * tc.BLOCK):
        step = slice(lo, lo + tc.SCAN_STEP * tc.BLOCK)
        assert (s3.buckets()[step] >= 2).any() and (s3.offsets[step] == len(s3.data)).any()
    big = [c for c in CASES if c.name.startswith("big_")]
    assert all(blocks(c) > tc.SCAN_STEP for c in big)  # a second step of the per-bucket scan and of the block sums
    assert any(c.n_buckets > 3 * tc.BUCKET_STEP for c in big)  # four steps of the bucket-base scan
    assert all(int(c.caplens.max()) <= 8 for c in big)
    t = tc.brute(BY_NAME["big_k255_drops"]).totals
    assert int(t[abi.STEER_DROPPED]) > tc.SCAN_STEP * 10
    t = tc.brute(BY_NAME["big_k7_keys_bad"]).totals
    assert int(t[abi.STEER_BAD_DESC]) > tc.SCAN_STEP
    assert {c.n_buckets for c in CASES} >= {1, 2, 3, 7, 8, 64, 255, 256}
    sp, sb = tc.steered_totals(BY_NAME["cap_exact"])
    exact = tc.brute(BY_NAME["cap_exact"]).totals
    assert [int(x) for x in exact[:5]] == [sp, sb, int(exact[abi.STEER_DROPPED]), 0, 0] and exact[abi.STEER_DROPPED] > 0
    for nm in OVERFLOWING:
        t = tc.brute(BY_NAME[nm]).totals
        assert [int(t[0]), int(t[1]), int(t[abi.STEER_OVERFLOW])] == [sp, sb, 1], nm
    for nm in ("index_only", "index_only_cap_ignored", "index_only_maxp_exact", "no_index"):
        assert int(tc.brute(BY_NAME[nm]).totals[abi.STEER_OVERFLOW]) == 0, nm
    for nm in ("bad_desc_random_k8", "bad_desc_some_dropped_k5"):
        assert int(tc.brute(BY_NAME[nm]).totals[abi.STEER_BAD_DESC]) > 20
    assert [int(x) for x in tc.brute(BY_NAME["bad_desc_all_dropped_k8"]).totals[:5]] == [0, 0, 900, 0, 0]
    c = BY_NAME["keys_k7_stride48"]  # % is a modulo: the edge keys land where Python says
    assert [int(k) % 7 for k in c.keys()[:5]] == [0, 1, 6, 0, 0xFFFFFFFF % 7] == list(c.buckets()[:5])
    rr = BY_NAME["pat_round_robin_k64"]
    assert len(set(rr.bucket[:64].tolist())) == 64  # every lane of a wave another bucket
    for c in CASES:
        if c.name.startswith("start") or c.name.startswith("grid_"):  # the last packet ends exactly at data_len
            assert int(c.offsets[-1]) + int(c.caplens[-1]) == c.dlen()
    grid = BY_NAME["grid_dst0"]
    assert {(int(ln), int(o) % 16) for ln, o in zip(grid.caplens, grid.offsets)} == \
        {(ln, a) for ln in range(48) for a in range(16)}


def test_steer_structs_match_header():
    fields = {"pcppx_steer_spec": abi.SteerSpec, "pcppx_steering": abi.Steering}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu\\n", sizeof(pcppx_steer_spec), sizeof(pcppx_steering));\n'
           '  printf("%d %d %d %d %d %d %d %d\\n", PCPPX_STEER_STEERED_PACKETS, PCPPX_STEER_STEERED_BYTES,\n'
           '         PCPPX_STEER_DROPPED, PCPPX_STEER_BAD_DESC, PCPPX_STEER_OVERFLOW, PCPPX_STEER_TOTALS,\n'
           '         PCPPX_STEER_MAX_BUCKETS, PCPPX_ABI_VERSION);\n' + lines + "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "s.c"
        c.write_text(src)
        exe = Path(d) / "s"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.SteerSpec), C.sizeof(abi.Steering)]
    assert [int(x) for x in out[1].split()] == [abi.STEER_STEERED_PACKETS, abi.STEER_STEERED_BYTES, abi.STEER_DROPPED,
                                                abi.STEER_BAD_DESC, abi.STEER_OVERFLOW, abi.STEER_TOTALS,
                                                abi.STEER_MAX_BUCKETS, abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        seen += 1
    assert seen == len(abi.SteerSpec._fields_) + len(abi.Steering._fields_)
    assert abi.ABI_VERSION == 7 and abi.STEER_FIELDS[abi.STEER_OVERFLOW] == "overflow"


def _good_args():
    b = abi.Batch(1, 1, 1, 1, 1, 1, 0)
    s = abi.make_steer_spec(bucket=1, n_buckets=8)
    o = abi.Steering(1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    return b, s, o


def _key_mode(s, key=4, stride=4):
    s.bucket, s.key, s.key_stride = None, key, stride


BAD_ARGS = {
    "null_totals": lambda b, s, o: setattr(o, "totals", None),
    "null_offsets": lambda b, s, o: setattr(o, "offsets", None),
    "null_caplens": lambda b, s, o: setattr(o, "caplens", None),
    "null_bucket_first": lambda b, s, o: setattr(o, "bucket_first", None),
    "null_bucket_pos": lambda b, s, o: setattr(o, "bucket_pos", None),
    "bucket_and_key_null": lambda b, s, o: setattr(s, "bucket", None),
    "bucket_and_key_set": lambda b, s, o: (setattr(s, "key", 4), setattr(s, "key_stride", 4)),
    "n_buckets_0": lambda b, s, o: setattr(s, "n_buckets", 0),
    "n_buckets_257": lambda b, s, o: setattr(s, "n_buckets", 257),
    "n_buckets_huge": lambda b, s, o: setattr(s, "n_buckets", 0xFFFFFFFF),
    "key_stride_0": lambda b, s, o: _key_mode(s, stride=0),
    "key_stride_2": lambda b, s, o: _key_mode(s, stride=2),
    "key_stride_6": lambda b, s, o: _key_mode(s, stride=6),
    "key_stride_33": lambda b, s, o: _key_mode(s, stride=33),
    "key_stride_260": lambda b, s, o: _key_mode(s, stride=260),
    "key_misaligned_1": lambda b, s, o: _key_mode(s, key=5),
    "key_misaligned_2": lambda b, s, o: _key_mode(s, key=6, stride=16),
    "spec_reserved": lambda b, s, o: setattr(s, "reserved", 1),
    "out_reserved": lambda b, s, o: setattr(o, "reserved", 1),
    "key_mode_spec_reserved": lambda b, s, o: (_key_mode(s), setattr(s, "reserved", 7)),
}


@pytest.mark.parametrize("what", sorted(BAD_ARGS))
def test_steer_rejects_bad_arguments_without_gpu(what):
    """PCPPX_E_INVAL before any device work: the context (address 1) is never dereferenced."""
    lib = abi.load_engine()
    ctx = C.c_void_p(1)
    b, s, o = _good_args()
    BAD_ARGS[what](b, s, o)
    assert lib.pcppx_steer_device(ctx, C.byref(b), C.byref(s), C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_steer_reference(C.byref(b), C.byref(s), C.byref(o)) == abi.E_INVAL


def test_steer_rejects_null_structs_without_gpu():
    lib = abi.load_engine()
    ctx = C.c_void_p(1)
    b, s, o = _good_args()
    assert lib.pcppx_steer_device(None, C.byref(b), C.byref(s), C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_steer_device(ctx, None, C.byref(s), C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_steer_device(ctx, C.byref(b), None, C.byref(o), None) == abi.E_INVAL
    assert lib.pcppx_steer_device(ctx, C.byref(b), C.byref(s), None, None) == abi.E_INVAL
    assert lib.pcppx_steer_reference(None, C.byref(s), C.byref(o)) == abi.E_INVAL
    assert lib.pcppx_steer_reference(C.byref(b), None, C.byref(o)) == abi.E_INVAL
    assert lib.pcppx_steer_reference(C.byref(b), C.byref(s), None) == abi.E_INVAL
    # the legal extremes pass the checks (reference: no context needed): both modes, K = 1 and 256, strides 4 and 256,
    # and an empty batch, which writes zero totals and all-zero bucket bounds
    for name in ("k1", "k256", "keys_k7_stride4", "keys_k7_stride256"):
        assert int(tc.run_reference(BY_NAME[name]).totals[abi.STEER_STEERED_PACKETS]) == BY_NAME[name].n
    for name in ("n0", "n0_k3_drops"):
        empty = tc.run_reference(BY_NAME[name])
        K = BY_NAME[name].n_buckets
        assert list(empty.totals) == [0] * abi.STEER_TOTALS
        assert not empty.bucket_first[:K + 1].any() and not empty.bucket_pos[:K + 1].any()


# ---- flow-exact sharding: the reason for the feature
FLOW_PORT = 5001


def _tcp(src: int, dst: int, sport: int, dport: int, flags: int) -> bytes:
    ip = struct.pack(">BBHHHBBH4s4s", 0x45, 0, 40, 0, 0, 64, 6, 0, src.to_bytes(4, "big"), dst.to_bytes(4, "big"))
    tcp = struct.pack(">HHIIBBHHH", sport, dport, 1, 1, 0x50, flags, 1024, 0, 0)
    return bytes(6) + bytes([2, 0, 0, 0, 0, 1]) + b"\x08\x00" + ip + tcp


def flow_stream(flows: int = 240) -> PacketBatch:
    """TCP flows each opened by a client->server packet to FLOW_PORT (it matches a dst_port spec); after the openers of
    every flow come the server->client packets, which match only through the flow table. A third of the flows talk to
    another port and never match."""
    rng = np.random.default_rng(5)
    cli = [(0x0A000000 + int(rng.integers(1, 1 << 16)), 0x0A010000 + int(rng.integers(1, 1 << 16)), 10000 + f,
            FLOW_PORT if f % 3 else 6000) for f in range(flows)]
    pk = [_tcp(s, d, sp, dp, 0x02) for s, d, sp, dp in cli]
    for rnd in range(2):
        for f in rng.permutation(flows):
            s, d, sp, dp = cli[int(f)]
            pk.append(_tcp(d, s, dp, sp, 0x12 if rnd == 0 else 0x10))
    return from_packets(pk)


def host_steer(batch: PacketBatch, keys: np.ndarray, K: int):
    """pcppx_steer_reference over a host batch by a u32 key column: (steered PacketBatch, index, bucket_first)."""
    c = tc.with_keys(tc.Case("host", batch.data, batch.offsets, batch.caplens, n_buckets=K), keys, 4, 0)
    r = tc.run_reference(c)
    n = int(r.totals[abi.STEER_STEERED_PACKETS])
    assert n == batch.n and int(r.totals[abi.STEER_OVERFLOW]) == 0
    out = PacketBatch(r.data[: int(r.totals[abi.STEER_STEERED_BYTES])], r.offsets[:n], r.caplens[:n], batch.linktype)
    return out, r.index[:n], r.bucket_first[: K + 1]


def bucket_view(out: PacketBatch, first, b: int) -> PacketBatch:
    from pcapplusplus_amd.engine import bucket_batch

    return bucket_batch(out, first, b)


def test_contiguous_sharding_changes_verdicts_and_steering_does_not():
    """The stream has teeth: two contiguous halves with separate flow tables miss the return direction of the flows
    opened in the first half; K buckets steered by hash5 (here by pcppx_steer_reference), each with its own table, give
    the single worker's verdicts and counters."""
    b = flow_stream()
    spec = oracle.make_spec(dst_port=FLOW_PORT)
    s, lay = oracle.oracle_parse(b, FILTER_OPTS)
    whole, wst = oracle.oracle_filter(b, s, lay, spec)
    assert 0 < int(whole.sum()) < b.n and int(whole[b.n // 2:].sum()) > 100
    half = b.n // 2
    m0, _ = oracle.oracle_filter(b.slice(0, half), s[:half], lay[:half], spec, {})
    m1, _ = oracle.oracle_filter(b.slice(half, b.n), s[half:], lay[half:], spec, {})
    assert not np.array_equal(np.concatenate([m0, m1]), whole)
    assert int(m1.sum()) == 0  # every return packet in the second half is missed
    for K in (2, 8):
        out, index, first = host_steer(b, s["hash5"], K)
        verdict = np.full(b.n, 2, np.uint8)
        st = {k: 0 for k in abi.STATS_FIELDS}
        for k in range(K):
            idx = index[int(first[k]):int(first[k + 1])]
            sub = bucket_view(out, first, k)
            assert [sub.packet(j) for j in range(sub.n)] == [b.packet(int(i)) for i in idx]
            m, bst = oracle.oracle_filter(sub, s[idx], lay[idx], spec, {})
            verdict[idx] = m
            st = {f: st[f] + bst[f] for f in st}
        assert np.array_equal(verdict, whole)
        assert all(st[f] == wst[f] for f in ("matched_packets", "matched_tcp_flows", "matched_udp_flows", "packet_count"))


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_steer_equals_reference(engine, case):
    got = tc.run_device(engine, case)
    tc.assert_same(got, tc.run_reference(case), case.name)
    if case.name in OVERFLOWING:
        assert int(got.totals[abi.STEER_OVERFLOW]) == 1
        tc.assert_untouched(got, case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["big_k256", "k7", "len_mix2000", "cap_short1"])
def test_gpu_steer_is_repeatable_across_streams(engine, name):
    """Two back-to-back calls on one context, on two streams (they share the context's scratch: the second waits for
    the first), into separate outputs: identical, and equal to the reference."""
    import torch

    case = BY_NAME[name]
    runs = [tc.DeviceRun(case), tc.DeviceRun(case)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for run, st in zip(runs, streams):
        run.launch(engine, st.cuda_stream)
    a, b = runs[0].result(), runs[1].result()
    tc.assert_same(a, b, name)
    tc.assert_same(a, tc.run_reference(case), name)


def _golden(stem):
    return load_golden(next(p for p in golden_files() if p.stem == stem))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("stem", ["synth_cfg3", "pcap_lt1"])
def test_gpu_steer_by_hash5_over_a_real_parse(engine, stem):
    """The key read through the summary, the brief, the tuples or the flow_keys column of a device parse: one output.
    Every bucket's hash5 % K is constant, and every bucket is an ordinary batch: its device parse equals the rows
    index[bucket] of the whole batch's parse, and the restatement's parse of it."""
    from pcapplusplus_amd.engine import bucket_batch, parse_on_device, parse_on_device_ex, steer_on_device

    b = _golden(stem)
    opts = abi.make_opts()
    rec = parse_on_device_ex(engine, b, opts, brief=True, tuples=True, flow_keys=True)
    fsum, flay = rec["summary"], rec["layers"]
    h5 = fsum["hash5"]
    assert np.array_equal(rec["brief"]["hash5"], h5) and np.array_equal(rec["flow_keys"], h5)
    for K in (3, 8):
        want = tc.run_reference(tc.with_keys(tc.Case(stem, b.data, b.offsets, b.caplens, n_buckets=K), h5, 4, 0))
        n = int(want.totals[abi.STEER_STEERED_PACKETS])
        assert n == b.n
        outs = [steer_on_device(engine, b, key=rec[src], n_buckets=K)
                for src in ("summary", "brief", "tuples", "flow_keys")]
        for out, index, first, pos, tot in outs:
            assert tot == dict(steered_packets=b.n, steered_bytes=b.wire_bytes(), dropped=0, bad_desc=0, overflow=0)
            assert np.array_equal(index, want.index[:n]) and np.array_equal(first, want.bucket_first[:K + 1])
            assert np.array_equal(pos, want.bucket_pos[:K + 1])
            assert np.array_equal(out.offsets, want.offsets[:n]) and np.array_equal(out.caplens, want.caplens[:n])
            assert out.data.tobytes() == want.data[:b.wire_bytes()].tobytes()
        out, index, first, pos, tot = outs[0]
        h2 = steer_on_device(engine, b, key=fsum, key_field="hash2", n_buckets=K, index_only=True)
        assert np.array_equal(np.sort(h2[1]), np.arange(b.n)) and len(h2[0].data) == 0
        for k in range(K):
            idx = index[int(first[k]):int(first[k + 1])]
            assert (h5[idx] % K == k).all() and (np.diff(idx.astype(np.int64)) > 0).all()
            assert (fsum["hash2"][h2[1][int(h2[2][k]):int(h2[2][k + 1])]] % K == k).all()
            sub = bucket_batch(out, first, k)
            if sub.n == 0:
                continue
            ssum, slay = parse_on_device(engine, sub.slice(0, sub.n), opts)
            oracle.compare_exact(ssum, slay, fsum[idx], flay[idx])
            osum, olay = oracle.oracle_parse(sub, opts)
            oracle.compare_exact(ssum, slay, osum, olay)
        assert np.array_equal(np.sort(index), np.arange(b.n))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 8])
def test_gpu_flow_exact_sharding(engine, K):
    """steer by hash5 -> pcppx_filter_device per bucket with its own zeroed flow table -> matched[] scattered back
    through index: the single worker's verdicts and counters, where contiguous halves give other verdicts."""
    from pcapplusplus_amd.engine import bucket_batch, parse_on_device, steer_on_device

    b = flow_stream()
    spec = oracle.make_spec(dst_port=FLOW_PORT)
    whole, wst = gpu_filter(engine, b, spec)
    s, lay = oracle.oracle_parse(b, FILTER_OPTS)
    assert np.array_equal(whole, oracle.oracle_filter(b, s, lay, spec)[0])
    half = b.n // 2
    halves = np.concatenate([gpu_filter(engine, b.slice(0, half), spec)[0], gpu_filter(engine, b.slice(half, b.n), spec)[0]])
    assert not np.array_equal(halves, whole)  # the contiguous split is wrong for this stream
    gsum, _ = parse_on_device(engine, b, FILTER_OPTS)
    out, index, first, pos, tot = steer_on_device(engine, b, key=gsum, n_buckets=K)
    assert tot["steered_packets"] == b.n and tot["overflow"] == 0
    verdict = np.full(b.n, 2, np.uint8)
    st = {k: 0 for k in abi.STATS_FIELDS}
    with_matches = 0
    for k in range(K):
        sub = bucket_batch(out, first, k)
        if sub.n == 0:
            continue
        m, bst = gpu_filter(engine, sub, spec)  # its own zeroed flow table
        verdict[index[int(first[k]):int(first[k + 1])]] = m
        st = {f: st[f] + bst[f] for f in st}
        with_matches += int(m.any())
    assert np.array_equal(verdict, whole)
    for f in ("matched_packets", "matched_tcp_flows", "matched_udp_flows", "packet_count", "tcp_count"):
        assert st[f] == wst[f], (f, st[f], wst[f])
    assert with_matches >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("stem,K", [("pcap_lt1", 4), ("synth_cfg3", 7)])
def test_gpu_steer_write_pcap(engine, stem, K, tmp_path):
    """steer -> D2H -> write_pcap of each bucket: together the K files hold every packet exactly once; within a file
    the packets are in capture order, with their timestamps and frame lengths."""
    from pcapplusplus_amd.engine import PcapReader, bucket_batch, parse_on_device, steer_on_device
    from pcapplusplus_amd.pcap import write_pcap

    b = _golden(stem)
    b = replace(b, timestamps_ns=(np.arange(b.n, dtype=np.uint64) + 1) * np.uint64(1_000_000),
                frame_lens=b.caplens + np.uint32(4))
    gsum, _ = parse_on_device(engine, b, FILTER_OPTS)
    out, index, first, pos, tot = steer_on_device(engine, b, key=gsum, n_buckets=K)
    seen = np.zeros(b.n, np.int64)
    for k in range(K):
        sub = bucket_batch(out, first, k)
        idx = index[int(first[k]):int(first[k + 1])]
        path = tmp_path / f"{stem}_{k}.pcap"
        write_pcap(path, sub)
        with PcapReader(str(path)) as rd:
            back = rd.read_batch(max_packets=sub.n + 1, data_cap=int(pos[k + 1] - pos[k]) + 64)
        assert back.n == len(idx) and back.linktype == b.linktype
        assert (np.diff(back.timestamps_ns.astype(np.int64)) > 0).all()  # capture order
        assert np.array_equal(back.timestamps_ns, b.timestamps_ns[idx])
        assert np.array_equal(back.frame_lens, b.frame_lens[idx])
        assert np.array_equal(back.caplens, b.caplens[idx])
        assert back.data[: int(back.caplens.sum())].tobytes() == b"".join(b.packet(int(i)) for i in idx)
        assert (gsum["hash5"][idx] % K == k).all()
        seen[idx] += 1
    assert (seen == 1).all()
