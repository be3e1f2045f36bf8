"""Case generators and runners for pcppx_select_device / pcppx_select_reference (tests/test_select.py).

A Case is a source batch (bytes + descriptors, possibly gapped, shuffled, overlapping or out of bounds), a selection
rule (a keep mask, or flags records + flags_any; invert; snaplen) and the output's capacities. Three runners produce
the same Buffers from it -- brute() (a per-packet Python loop: the contract of include/pcppx.h restated),
run_reference() (pcppx_select_reference) and run_device() (pcppx_select_device) -- every buffer pre-filled with 0xA5
and over-allocated by 64 B / 4 entries, so equality of the whole buffers also shows that nothing beyond WRITTEN_* was
touched.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import mover_cases as mc
from mover_cases import FILL, PAD_BYTES, PAD_ENTRIES, mix_lens, packed  # noqa: F401  (the tests read them here)
from pcapplusplus_amd import abi

BLOCK = 1024  # packets per block of the count and copy kernels (pcppx_internal.h kSelectBlockPk)
BASE_STEP = 256  # block sums per step of select_base_kernel's scan (one wave, four consecutive blocks per lane)
SCAN3_N = 2 * BASE_STEP * BLOCK + 1029  # two whole steps of that scan, then a block and a partial one
FIELDS = ("offsets", "caplens", "index", "data")


@dataclass
class Case(mc.Case):
    keep: np.ndarray | None = None    # u8[n]; None = flags mode
    flags: np.ndarray | None = None   # flags mode: the records' bytes (u8, n * flags_stride)
    flags_stride: int = 0
    flags_any: int = 0
    invert: bool = False


@dataclass
class Buffers(mc.Buffers):
    totals: np.ndarray


def alloc(c: Case) -> Buffers:
    return Buffers(*mc.alloc(c), np.full(abi.SEL_TOTALS, mc.F64, np.uint64))


def chosen(c: Case) -> np.ndarray:
    """The keep rule alone (before the bounds check), as booleans."""
    if c.keep is not None:
        k = c.keep != 0
    else:
        rec = c.flags.reshape(c.n, c.flags_stride) if c.n else np.zeros((0, c.flags_stride), np.uint8)
        fl = rec[:, abi.FLAGS_OFFSET].astype(np.uint16) | (rec[:, abi.FLAGS_OFFSET + 1].astype(np.uint16) << 8)
        k = (fl & c.flags_any) != 0
    return ~k if c.invert else k


def brute(c: Case) -> Buffers:
    """include/pcppx.h's select contract, one packet at a time."""
    out = alloc(c)
    ch = chosen(c)
    sel = sel_bytes = written = written_bytes = bad = 0
    open_ = True
    data_len, data_cap, max_packets = c.dlen(), c.cap(), c.maxp()
    for i in np.nonzero(ch)[0]:
        off, cap = int(c.offsets[i]), int(c.caplens[i])
        if off + cap > data_len:  # Python integers: no wrap (the C code checks the 64-bit wrap too)
            bad += 1
            continue
        ln = min(cap, c.snaplen) if c.snaplen else cap
        open_ = open_ and sel < max_packets and (c.index_only or sel_bytes + ln <= data_cap)
        if open_:
            out.offsets[sel] = sel_bytes
            out.caplens[sel] = ln
            if out.index is not None:
                out.index[sel] = i
            if not c.index_only:
                out.data[sel_bytes:sel_bytes + ln] = c.data[off:off + ln]
            written += 1
            written_bytes += ln
        sel += 1
        sel_bytes += ln
    out.totals[:] = 0
    out.totals[:5] = (sel, sel_bytes, written, written_bytes, bad)
    return out


def _spec(c: Case, keep_addr, flags_addr) -> abi.SelectSpec:
    if c.keep is not None:
        return abi.make_select_spec(keep=keep_addr, invert=c.invert, snaplen=c.snaplen)
    return abi.make_select_spec(flags=flags_addr + abi.FLAGS_OFFSET, flags_stride=c.flags_stride,
                                flags_any=c.flags_any, invert=c.invert, snaplen=c.snaplen)


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    keep = np.ascontiguousarray(c.keep if c.keep is not None else c.flags)
    keep = keep if len(keep) else np.zeros(16, np.uint8)  # a non-null address for an empty batch
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, 1, 0)
    sel = abi.Selection(None if c.index_only else out.data.ctypes.data, c.cap(), out.offsets.ctypes.data,
                        out.caplens.ctypes.data, out.index.ctypes.data if out.index is not None else None, c.maxp(), 0,
                        out.totals.ctypes.data)
    abi.select_reference(b, _spec(c, keep.ctypes.data, keep.ctypes.data), sel)
    return out


def run_device(engine, c: Case, device: str = "cuda:0", source=None) -> Buffers:
    """source: see mover_cases.Staged."""
    import torch

    host = alloc(c)
    dev = mc.Staged(c, host, device, source)
    rule = np.ascontiguousarray(c.keep if c.keep is not None else c.flags)
    rule_t = dev.up(rule if len(rule) else np.zeros(16, np.uint8))
    d_tot = dev.up(host.totals.view(np.int64))
    engine.select_device(dev.data, dev.offsets, dev.caplens, c.n, 1, _spec(c, abi.ptr(rule_t), abi.ptr(rule_t)),
                         dev.d_off, dev.d_cap, d_tot, c.maxp(), dev.d_data, c.cap(), dev.d_idx,
                         torch.cuda.current_stream(device).cuda_stream, data_len=dev.data_len)
    return Buffers(*dev.common(), dev.down(d_tot, np.uint64))


def assert_same(got: Buffers, want: Buffers, what: str) -> None:
    mc.assert_same(got, want, what, FIELDS)


# ------------------------------------------------------------------ generators
def mask(n: int, pattern: str, seed: int = 0) -> np.ndarray:
    k = np.zeros(n, np.uint8)
    rng = np.random.default_rng(seed)
    if pattern == "all":
        k[:] = 1
    elif pattern == "alt":
        k[::2] = 0x80  # any non-zero byte selects
    elif pattern == "first" and n:
        k[0] = 1
    elif pattern == "last" and n:
        k[-1] = 1
    elif pattern == "p1":
        k[:] = rng.random(n) < 0.01
    elif pattern == "p50":
        k[:] = rng.random(n) < 0.5
    elif pattern == "hole":  # tiles 0 and 2 kept, tile 1 (and the rest) empty
        k[:64] = 1
        k[128:192] = 1
    return k


def make(name: str, lens, pattern: str = "p50", seed: int = 1, **kw) -> Case:
    layout = {k: kw.pop(k) for k in ("start", "gaps", "tail") if k in kw}
    data, offs, lens = packed(lens, seed, **layout)
    return Case(name, data, offs, lens, keep=mask(len(lens), pattern, seed + 100), **kw)


def selected_totals(c: Case):
    t = brute(replace(c, data_cap=None, max_packets=None, index_only=True)).totals
    return int(t[abi.SEL_SELECTED_PACKETS]), int(t[abi.SEL_SELECTED_BYTES])


def cases() -> list[Case]:
    out: list[Case] = []
    # n: the tile and block edges, and 42 / 91 blocks for the block-base scan (one wave, four consecutive blocks per lane:
    # 23 lanes carry into each other at 91). scan3 (1-8 B packets, so half a million of them stay small in bytes) runs the
    # scan through two whole 256-block steps and a partial third one; tests/test_wide_offsets.py goes on to dozens of
    # steps with an output past 2^32.
    for n in (0, 1, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, 41 * BLOCK + 7, 90 * BLOCK + 5):
        out.append(make(f"n{n}", mix_lens(n, 40, n), "p50", seed=n))
    out.append(make("scan3", np.random.default_rng(12).integers(1, 9, SCAN3_N).astype(np.uint32), "p50", seed=12))
    out.append(make("n_big_p1", mix_lens(90 * BLOCK + 5, 40, 9), "p1", seed=9))
    out.append(make("n_big_all", mix_lens(66 * BLOCK + 3, 90, 10), "all", seed=10))
    # keep patterns
    for pat in ("none", "all", "alt", "first", "last", "p1", "p50", "hole"):
        out.append(make(f"keep_{pat}", mix_lens(1000, 300, 3), pat, seed=3))
    for pat in ("alt", "p1", "all", "none"):
        out.append(make(f"invert_{pat}", mix_lens(1000, 300, 4), pat, seed=4, invert=True))
    # lengths
    out.append(make("len_0_33_all", np.tile(np.arange(34), 20), "all", seed=5))
    out.append(make("len_0_33_p50", np.tile(np.arange(34), 20), "p50", seed=6))
    for ln in (64, 512, 1500):
        out.append(make(f"len_{ln}", np.full(300, ln), "p50", seed=ln))
        out.append(make(f"len_{ln}_all", np.full(130, ln), "all", seed=ln + 1))
    out.append(make("len_jumbo", [64, 64, 65535, 64, 70000, 64, 64], "all", seed=7))
    out.append(make("len_jumbo_alt", [64, 64, 65535, 64, 70000, 64, 64, 3], "alt", seed=7))
    out.append(make("len_mix2000", mix_lens(1000, 2000, 8), "p50", seed=8))
    out.append(make("len_mix2000_all", mix_lens(700, 2000, 18), "all", seed=18))
    # source layout: every source alignment, gaps, unordered and overlapping descriptors; `tail` 0 everywhere, so the
    # last packet ends exactly at data_len
    for s in range(16):
        out.append(make(f"start{s}", mix_lens(200, 100, 20 + s), "p50", seed=20 + s, start=s))
    out.append(make("gapped", mix_lens(600, 200, 40), "p50", seed=40, gaps=mix_lens(600, 40, 41)))
    out.append(mc.shuffled(make("shuffled", mix_lens(600, 200, 42), "p50", seed=42), 43))
    c = mc.overlapped(make("overlap", mix_lens(300, 200, 44), "all", seed=44))
    out.append(replace(c, keep=mask(c.n, "p50", 45)))
    for mis in (1, 7, 15):  # a destination that does not start on a 16-B boundary
        out.append(make(f"dst_misaligned{mis}", mix_lens(400, 150, 46 + mis), "p50", seed=46 + mis, out_misalign=mis))
    # snaplen
    for sn in (1, 14, 60, 64, 5000):
        out.append(make(f"snap{sn}", mix_lens(500, 200, 50), "p50", seed=50, snaplen=sn))
    out.append(make("snap96_1500", np.full(200, 1500), "all", seed=51, snaplen=96))
    # capacity
    base = make("cap", np.maximum(mix_lens(700, 300, 60), 1), "p50", seed=60)  # no empty packet: one byte short drops one
    sp, sb = selected_totals(base)
    for nm, kw in (("cap_exact", dict(data_cap=sb)), ("cap_short1", dict(data_cap=sb - 1)),
                   ("cap_half", dict(data_cap=sb // 2)), ("cap_zero", dict(data_cap=0)),
                   ("maxp_exact", dict(max_packets=sp)), ("maxp_short1", dict(max_packets=sp - 1)),
                   ("maxp_zero", dict(max_packets=0)), ("maxp_half_cap_half", dict(max_packets=sp // 2, data_cap=sb // 2)),
                   ("index_only", dict(index_only=True)), ("index_only_cap_ignored", dict(index_only=True, data_cap=5)),
                   ("index_only_maxp", dict(index_only=True, max_packets=sp // 3)), ("no_index", dict(want_index=False))):
        out.append(replace(base, name=nm, **kw))
    for pat in ("all", "p50"):
        out.append(mc.with_bad_descriptors(make(f"bad_desc_{pat}", mix_lens(900, 120, 70), pat, seed=70)))
    # flags mode over synthetic records (the device tests also run it over a real parse's records)
    for stride in (16, 32):
        c = make(f"flags_stride{stride}", mix_lens(800, 150, 80), "none", seed=80)
        rec = np.random.default_rng(81).integers(0, 256, c.n * stride, dtype=np.uint8)
        out.append(replace(c, keep=None, flags=rec, flags_stride=stride, flags_any=abi.F_NEEDS_HOST))
        out.append(replace(c, name=c.name + "_inv_snap", keep=None, flags=rec, flags_stride=stride, flags_any=0x0101,
                           invert=True, snaplen=60))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
