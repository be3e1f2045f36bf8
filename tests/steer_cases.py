"""Case generators and runners for pcppx_steer_device / pcppx_steer_reference (tests/test_steer.py).

A Case is a source batch (bytes + descriptors, possibly gapped, shuffled, overlapping or out of bounds), a steering
rule (a bucket column, or key records + stride + offset; n_buckets; snaplen) and the output's capacities. Three runners
produce the same Buffers from it -- brute() (a per-packet Python loop: the contract of include/pcppx.h restated),
run_reference() (pcppx_steer_reference) and run_device() (pcppx_steer_device) -- every buffer pre-filled with 0xA5 and
over-allocated by 64 B / 4 entries, so equality of the whole buffers also shows that nothing beyond STEERED_* was
touched, and nothing at all on overflow.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import mover_cases as mc
from mover_cases import F32, F64, FILL, mix_lens, packed
from pcapplusplus_amd import abi
from select_cases import SCAN3_N

BLOCK = 1024    # packets per block of the count and copy kernels (pcppx_internal.h kSteerBlockPk)
SCAN_STEP = 64  # block sums per step of the per-bucket scan (pcppx_internal.h kSteerScanStep)
BUCKET_STEP = 64  # buckets per step of the one-wave bucket-base scan (one per lane)


@dataclass
class Case(mc.Case):
    n_buckets: int = 1
    bucket: np.ndarray | None = None  # u8[n]; None = key mode
    key: np.ndarray | None = None     # key mode: the records' bytes (u8, n * key_stride), the key at key_offset
    key_stride: int = 4
    key_offset: int = 0
    src_misalign: int = 0             # device runs: batch->data starts this many bytes past a 16-B boundary

    def keys(self) -> np.ndarray:
        """Key mode: the n 32-bit keys."""
        rec = self.key[: self.n * self.key_stride].reshape(self.n, self.key_stride)
        return np.ascontiguousarray(rec[:, self.key_offset:self.key_offset + 4]).view("<u4").reshape(-1)

    def buckets(self) -> np.ndarray:
        """The rule alone (before the bounds check): every packet's bucket value as an integer (>= n_buckets: dropped)."""
        if self.bucket is not None:
            return self.bucket.astype(np.int64)
        return (self.keys() % np.uint32(self.n_buckets)).astype(np.int64)


@dataclass
class Buffers(mc.Buffers):
    bucket_first: np.ndarray
    bucket_pos: np.ndarray
    totals: np.ndarray


FIELDS = ("offsets", "caplens", "index", "bucket_first", "bucket_pos", "data")


def alloc(c: Case) -> Buffers:
    return Buffers(*mc.alloc(c), np.full(c.n_buckets + 1 + mc.PAD_ENTRIES, F32, np.uint32),
                   np.full(c.n_buckets + 1 + mc.PAD_ENTRIES, F64, np.uint64), np.full(abi.STEER_TOTALS, F64, np.uint64))


def brute(c: Case) -> Buffers:
    """include/pcppx.h's steer contract, one packet at a time."""
    out = alloc(c)
    K, data_len = c.n_buckets, c.dlen()
    per = [[] for _ in range(K)]  # per bucket: (source packet, source offset, output length), in source order
    dropped = bad = 0
    for i, v in enumerate(c.buckets().tolist()):
        if v >= K:
            dropped += 1  # its descriptor is not looked at
            continue
        off, cap = int(c.offsets[i]), int(c.caplens[i])
        if off + cap > data_len:  # Python integers: no wrap (the C code checks the 64-bit wrap too)
            bad += 1
            continue
        per[v].append((i, off, min(cap, c.snaplen) if c.snaplen else cap))
    r = p = 0
    for b in range(K):
        out.bucket_first[b], out.bucket_pos[b] = r, p
        r += len(per[b])
        p += sum(x[2] for x in per[b])
    out.bucket_first[K], out.bucket_pos[K] = r, p
    overflow = r > c.maxp() or (not c.index_only and p > c.cap())
    out.totals[:] = 0
    out.totals[:5] = (r, p, dropped, bad, int(overflow))
    if overflow:
        return out
    r = p = 0
    for b in range(K):
        for i, off, ln in per[b]:
            out.offsets[r] = p
            out.caplens[r] = ln
            if out.index is not None:
                out.index[r] = i
            if not c.index_only:
                out.data[p:p + ln] = c.data[off:off + ln]
            r += 1
            p += ln
    return out


def _rule(c: Case) -> np.ndarray:
    rule = np.ascontiguousarray(c.bucket if c.bucket is not None else c.key)
    return rule if len(rule) else np.zeros(64, np.uint8)  # a non-null address for an empty batch


def _spec(c: Case, addr: int) -> abi.SteerSpec:
    if c.bucket is not None:
        return abi.make_steer_spec(bucket=addr, n_buckets=c.n_buckets, snaplen=c.snaplen)
    return abi.make_steer_spec(key=addr + c.key_offset, key_stride=c.key_stride, n_buckets=c.n_buckets,
                               snaplen=c.snaplen)


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    rule = _rule(c)
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, 1, 0)
    st = abi.Steering(None if c.index_only else out.data.ctypes.data, c.cap(), out.offsets.ctypes.data,
                      out.caplens.ctypes.data, out.index.ctypes.data if out.index is not None else None,
                      out.bucket_first.ctypes.data, out.bucket_pos.ctypes.data, c.maxp(), 0, out.totals.ctypes.data)
    abi.steer_reference(b, _spec(c, rule.ctypes.data), st)
    return out


class DeviceRun(mc.Staged):
    """A case's tensors on the device; launch() queues pcppx_steer_device on a stream, result() reads the buffers."""

    def __init__(self, c: Case, device: str = "cuda:0", source=None):
        """source: see mover_cases.Staged."""
        host = alloc(c)
        super().__init__(c, host, device, source, c.src_misalign)
        self.rule = self.up(_rule(c))
        self.d_first, self.d_pos = self.up(host.bucket_first.view(np.int32)), self.up(host.bucket_pos.view(np.int64))
        self.d_tot = self.up(host.totals.view(np.int64))

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.steer_device(self.data, self.offsets, self.caplens, c.n, 1, _spec(c, abi.ptr(self.rule)), self.d_off,
                            self.d_cap, self.d_first, self.d_pos, self.d_tot, c.maxp(), self.d_data, c.cap(), self.d_idx,
                            stream, data_len=self.data_len)

    def result(self) -> Buffers:
        return Buffers(*self.common(), self.down(self.d_first, np.uint32), self.down(self.d_pos, np.uint64),
                       self.down(self.d_tot, np.uint64))


def run_device(engine, c: Case, device: str = "cuda:0", source=None) -> Buffers:
    import torch

    run = DeviceRun(c, device, source)
    run.launch(engine, torch.cuda.current_stream(device).cuda_stream)
    return run.result()


def assert_same(got: Buffers, want: Buffers, what: str) -> None:
    mc.assert_same(got, want, what, FIELDS)


def assert_untouched(got: Buffers, what: str) -> None:
    """The all-or-nothing rule: data, offsets, caplens and index still hold the fill, every byte of them."""
    for f, fill in (("data", FILL), ("offsets", F64), ("caplens", F32), ("index", F32)):
        g = getattr(got, f)
        assert g is None or bool((g == fill).all()), (what, f)


# ------------------------------------------------------------------ generators
def column(n: int, K: int, pattern: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    if pattern == "random":
        b = rng.integers(0, K, n)
    elif pattern == "one":        # all packets in one (a middle) bucket
        b = np.full(n, K // 2)
    elif pattern == "first_empty":
        b = rng.integers(1, K, n) if K > 1 else np.zeros(n)
    elif pattern == "last_empty":
        b = rng.integers(0, max(K - 1, 1), n)
    elif pattern == "middle_empty":
        b = rng.integers(0, max(K - 1, 1), n)
        b[b >= K // 2] += 1
    elif pattern == "round_robin":  # every lane of a wave another bucket (K >= 64)
        b = i % K
    elif pattern == "sorted":
        b = np.sort(rng.integers(0, K, n))
    elif pattern == "reverse":
        b = np.sort(rng.integers(0, K, n))[::-1]
    elif pattern == "single_last":  # one packet in the last bucket, the rest in bucket 0
        b = np.zeros(n)
        b[n // 2] = K - 1
    elif pattern == "some_dropped":  # values >= K, 255 among them
        b = rng.integers(0, K, n)
        b[rng.random(n) < 0.2] = K
        b[rng.random(n) < 0.1] = 255
        b[rng.random(n) < 0.05] = min(K + 100, 255)
    elif pattern == "all_dropped":
        b = np.where(i % 2 == 0, K, 255)
    else:
        raise ValueError(pattern)
    return np.asarray(b).astype(np.uint8)


def make(name: str, lens, K: int = 8, pattern: str = "random", seed: int = 1, **kw) -> Case:
    layout = {k: kw.pop(k) for k in ("start", "gaps", "tail") if k in kw}
    data, offs, lens = packed(lens, seed, **layout)
    return Case(name, data, offs, lens, n_buckets=K, bucket=column(len(lens), K, pattern, seed + 100), **kw)


def with_keys(c: Case, keys: np.ndarray, stride: int, offset: int, seed: int = 5) -> Case:
    """The same batch in key mode: random records of `stride` bytes with the 32-bit key at `offset`."""
    rec = np.random.default_rng(seed).integers(0, 256, (c.n, stride), dtype=np.uint8)
    rec[:, offset:offset + 4] = np.ascontiguousarray(keys.astype("<u4")).view(np.uint8).reshape(c.n, 4)
    return replace(c, bucket=None, key=rec.reshape(-1), key_stride=stride, key_offset=offset)


def steered_totals(c: Case):
    t = brute(replace(c, data_cap=None, max_packets=None, index_only=True)).totals
    return int(t[abi.STEER_STEERED_PACKETS]), int(t[abi.STEER_STEERED_BYTES])


def small_lens(n: int, seed: int) -> np.ndarray:
    """1-8 B packets: the large-n cases stay small in bytes."""
    return np.random.default_rng(seed).integers(1, 9, n).astype(np.uint32)


def aligned_grid() -> tuple[list[int], list[int]]:
    """Lengths 0-47, each at all 16 source alignments: (lens, gaps) for packed()."""
    lens, gaps, pos = [], [], 0
    for ln in range(48):
        for a in range(16):
            gap = (a - pos) % 16
            lens.append(ln)
            gaps.append(gap)
            pos += gap + ln
    return lens, gaps


BIG_N = (SCAN_STEP + 6) * BLOCK + 5  # 70 blocks and a partial one: every scan loop runs a second step


def cases() -> list[Case]:
    out: list[Case] = []
    # n: the tile and block edges
    for n in (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5):
        out.append(make(f"n{n}", mix_lens(n, 40, n), 8, "random", seed=n))
        out.append(make(f"n{n}_k3_drops", mix_lens(n, 40, n + 1), 3, "some_dropped", seed=n + 1))
    # more blocks than one step of the per-bucket scan and of the dropped / bad sums, more buckets than one step of the
    # bucket-base scan: each of those loops carries into a second step
    out.append(make("big_k256", small_lens(BIG_N, 9), 256, "random", seed=9))
    out.append(make("big_k255_drops", small_lens(BIG_N, 10), 255, "some_dropped", seed=10))
    out.append(make("big_k8_rr", small_lens(BIG_N, 11), 8, "round_robin", seed=11))
    c = make("big_k7_keys_bad", small_lens(BIG_N, 12), 7, "random", seed=12)
    offs = c.offsets.copy()
    offs[3::997] = np.uint64(len(c.data))  # bad descriptors in many blocks (every length is >= 1)
    out.append(with_keys(replace(c, offsets=offs), np.random.default_rng(13).integers(0, 1 << 32, c.n), 16, 4))
    # the n of select_cases' scan3 (513 blocks and a partial one): nine steps of the per-bucket scan and of the dropped /
    # bad sums, with dropped and bad packets in every step
    c = make("scan3_k2_drops_bad", small_lens(SCAN3_N, 14), 2, "some_dropped", seed=14)
    offs = c.offsets.copy()
    offs[3::997] = np.uint64(len(c.data))
    out.append(replace(c, offsets=offs))
    # K
    for K in (1, 2, 3, 7, 8, 64, 255, 256):
        out.append(make(f"k{K}", mix_lens(1500, 100, K), K, "random", seed=K))
    # bucket patterns
    for K, pat in ((8, "one"), (8, "first_empty"), (8, "last_empty"), (8, "middle_empty"), (3, "middle_empty"),
                   (64, "round_robin"), (256, "round_robin"), (7, "round_robin"), (8, "sorted"), (8, "reverse"),
                   (256, "sorted"), (64, "reverse"), (8, "single_last"), (256, "single_last"), (8, "some_dropped"),
                   (2, "some_dropped"), (255, "some_dropped"), (8, "all_dropped"), (1, "all_dropped")):
        out.append(make(f"pat_{pat}_k{K}", mix_lens(1300, 120, K + 30), K, pat, seed=K + 30))
    # key mode: K not a power of two, so that % is a modulo; the edge keys; every stride, the key inside the record
    for K in (7, 255, 3):
        base = make(f"keys_k{K}", mix_lens(900, 90, K + 60), K, "random", seed=K + 60)
        keys = np.random.default_rng(K).integers(0, 1 << 32, base.n, dtype=np.uint64)
        keys[:10] = [0, 1, K - 1, K, 0xFFFFFFFF, K + 1, 2 * K, 2 * K - 1, 0xFFFFFFFE, 0x80000000]
        keys[-5:] = [0xFFFFFFFF, K, K - 1, 1, 0]
        for stride, off in ((4, 0), (16, 4), (32, 8), (48, 40), (256, 252)):
            out.append(replace(with_keys(base, keys, stride, off), name=f"keys_k{K}_stride{stride}"))
    out.append(replace(with_keys(make("keys_k8_snap", mix_lens(500, 200, 77), 8, seed=77),
                                 np.arange(500) * 2654435761 % (1 << 32), 32, 0), snaplen=60))
    # lengths 0-47 at all 16 source alignments, crossed with destination misalignments (and a misaligned source base)
    lens, gaps = aligned_grid()
    for mis in (0, 1, 7, 15):
        out.append(make(f"grid_dst{mis}", lens, 3, "random", seed=80 + mis, gaps=gaps, out_misalign=mis))
        out.append(make(f"grid_dst{mis}_k1", lens, 1, "random", seed=90 + mis, gaps=gaps, out_misalign=mis))
    out.append(make("grid_src5_dst9", lens, 5, "random", seed=99, gaps=gaps, out_misalign=9, src_misalign=5))
    for s in (1, 8, 15):
        out.append(make(f"start{s}", mix_lens(300, 100, 20 + s), 4, "random", seed=20 + s, start=s))
    # runs of zero-length packets
    z = mix_lens(1200, 60, 33)
    z[100:300] = 0
    z[640:705] = 0
    z[-70:] = 0
    out.append(make("zero_runs", z, 5, "random", seed=33))
    out.append(make("all_zero_len", np.zeros(700, np.uint32), 6, "random", seed=34))
    # long packets
    out.append(make("len_jumbo", [64, 9000, 64, 65535, 64, 70000, 64, 9000, 3], 2, "random", seed=7))
    out.append(make("len_jumbo_k1", [9000, 65535, 70000], 1, "random", seed=8))
    out.append(make("len_jumbo_rev", [64, 9000, 64, 65535, 64, 70000, 64, 9000, 3], 3, "reverse", seed=7,
                    out_misalign=3))
    out.append(make("len_mix2000", mix_lens(900, 2000, 8), 8, "random", seed=8))
    for ln in (64, 512, 1500):
        out.append(make(f"len_{ln}", np.full(200, ln), 8, "random", seed=ln))
    # source layout: gaps, unordered and overlapping descriptors; `tail` 0 everywhere, so the last packet ends exactly at
    # data_len
    out.append(make("gapped", mix_lens(600, 200, 40), 8, "random", seed=40, gaps=mix_lens(600, 40, 41)))
    out.append(mc.shuffled(make("shuffled", mix_lens(600, 200, 42), 8, "random", seed=42), 43))
    c = mc.overlapped(make("overlap", mix_lens(300, 200, 44), 8, "random", seed=44))
    out.append(replace(c, bucket=column(c.n, 8, "random", 45)))
    # bad descriptors, inside steered buckets and inside dropped ones
    for K, pat in ((8, "random"), (5, "some_dropped"), (8, "all_dropped")):
        out.append(mc.with_bad_descriptors(make(f"bad_desc_{pat}_k{K}", mix_lens(900, 120, 70), K, pat, seed=70)))
    # snaplen below, at and above the packet sizes
    for sn in (1, 14, 60, 64, 200, 5000):
        out.append(make(f"snap{sn}", mix_lens(500, 200, 50), 8, "random", seed=50, snaplen=sn))
    out.append(make("snap96_1500", np.full(200, 1500), 4, "random", seed=51, snaplen=96))
    # capacity: all or nothing
    base = make("cap", np.maximum(mix_lens(700, 300, 60), 1), 8, "some_dropped", seed=60)
    sp, sb = steered_totals(base)
    for nm, kw in (("cap_exact", dict(data_cap=sb, max_packets=sp)), ("cap_short1", dict(data_cap=sb - 1)),
                   ("cap_half", dict(data_cap=sb // 2)), ("cap_zero", dict(data_cap=0)),
                   ("maxp_short1", dict(max_packets=sp - 1)), ("maxp_zero", dict(max_packets=0)),
                   ("cap_zero_maxp_zero", dict(max_packets=0, data_cap=0)),
                   ("index_only", dict(index_only=True)), ("index_only_cap_ignored", dict(index_only=True, data_cap=5)),
                   ("index_only_maxp_exact", dict(index_only=True, max_packets=sp)),
                   ("index_only_maxp_short1", dict(index_only=True, max_packets=sp - 1)),
                   ("no_index", dict(want_index=False)), ("no_index_overflow", dict(want_index=False, data_cap=sb - 1))):
        out.append(replace(base, name=nm, **kw))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
