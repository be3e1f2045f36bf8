"""What the case modules of the operators that move packets of a device batch share (select_cases.py, steer_cases.py).

A case is a source batch (bytes + descriptors, possibly gapped, shuffled, overlapping or out of bounds), the operator's
own rule and the output's capacities. Every output buffer is pre-filled with 0xA5 and over-allocated by 64 B / 4
entries, so equality of the whole buffers also shows that nothing beyond the written part was touched.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

FILL, F32, F64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
PAD_BYTES, PAD_ENTRIES = 64, 4


@dataclass
class Case:
    name: str
    data: np.ndarray      # u8
    offsets: np.ndarray   # u64
    caplens: np.ndarray   # u32
    snaplen: int = 0
    data_len: int | None = None       # None: len(data)
    data_cap: int | None = None       # None: the bytes of the whole batch (always enough)
    max_packets: int | None = None    # None: n
    index_only: bool = False
    want_index: bool = True
    out_misalign: int = 0             # device runs: out->data starts this many bytes past a 16-B boundary
    meta: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return len(self.caplens)

    def dlen(self) -> int:
        return len(self.data) if self.data_len is None else self.data_len

    def cap(self) -> int:
        if self.data_cap is not None:
            return self.data_cap
        dl = np.uint64(self.dlen())
        room = dl - np.minimum(self.offsets, dl)  # no 64-bit wrap: the bytes from the offset to data_len
        ok = (self.offsets <= dl) & (self.caplens.astype(np.uint64) <= room)  # the in-bounds packets
        return int(self.caplens[ok].astype(np.uint64).sum())

    def maxp(self) -> int:
        return self.n if self.max_packets is None else self.max_packets


@dataclass
class Buffers:
    data: np.ndarray | None
    offsets: np.ndarray
    caplens: np.ndarray
    index: np.ndarray | None


def alloc(c: Case) -> tuple:
    """The filled data, offsets, caplens and index arrays of a case's output."""
    return (None if c.index_only else np.full(c.cap() + PAD_BYTES, FILL, np.uint8),
            np.full(c.maxp() + PAD_ENTRIES, F64, np.uint64),
            np.full(c.maxp() + PAD_ENTRIES, F32, np.uint32),
            np.full(c.maxp() + PAD_ENTRIES, F32, np.uint32) if c.want_index else None)


def assert_same(got, want, what: str, fields) -> None:
    """Whole buffers, pads included: the written part equal, the 0xA5 fill intact everywhere else."""
    assert list(got.totals) == list(want.totals), (what, "totals", list(got.totals), list(want.totals))
    for f in fields:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), (what, f)
        if g is None:
            continue
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, f, len(bad), "first at", int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


class Staged:
    """A case's source batch and the common output arrays on the device, out->data behind a filled guard band."""

    def __init__(self, c: Case, host: Buffers, device: str, source=None, src_misalign: int = 0):
        """source: (data, offsets, caplens, data_len) tensors already on the device to read from instead of c's own
        batch (c then holds the rule, the capacities and, for the runners on the host, the same packets in a small
        buffer). src_misalign: c's own batch starts this many bytes past a 16-B boundary."""
        self.c, self.device = c, device
        if source is None:
            src = c.data if len(c.data) else np.zeros(1, np.uint8)
            self.s_raw = self.up(np.concatenate([np.zeros(16 + src_misalign, np.uint8), src]))
            self.data = self.s_raw[16 + src_misalign:]
            assert self.data.data_ptr() % 16 == src_misalign
            self.offsets, self.caplens = self.up(c.offsets.view(np.int64)), self.up(c.caplens.view(np.int32))
            self.data_len = c.dlen()
        else:
            self.data, self.offsets, self.caplens, self.data_len = source
        self.guard = 16 + c.out_misalign
        self.d_raw = None if c.index_only else self.up(np.concatenate([np.full(self.guard, FILL, np.uint8), host.data]))
        self.d_data = None if c.index_only else self.d_raw[self.guard:]
        if self.d_data is not None:
            assert self.d_data.data_ptr() % 16 == c.out_misalign
        self.d_off, self.d_cap = self.up(host.offsets.view(np.int64)), self.up(host.caplens.view(np.int32))
        self.d_idx = self.up(host.index.view(np.int32)) if host.index is not None else None

    def up(self, a: np.ndarray):
        import torch

        return torch.from_numpy(a).to(self.device)

    @staticmethod
    def down(t, dtype):
        return None if t is None else t.cpu().numpy().view(dtype)

    def common(self) -> tuple:
        """After the device's work: the guard band checked, then the data, offsets, caplens and index arrays."""
        import torch

        torch.cuda.synchronize(self.device)
        if self.d_raw is not None:  # the bytes in front of out->data belong to someone else
            assert bool((self.d_raw[:self.guard] == FILL).all()), "bytes before out->data were written"
        return (self.down(self.d_data, np.uint8), self.down(self.d_off, np.uint64), self.down(self.d_cap, np.uint32),
                self.down(self.d_idx, np.uint32))


# ------------------------------------------------------------------ generators
def packed(lens, seed: int, start: int = 0, gaps=None, tail: int = 0):
    """Packets of the given lengths, back to back from byte `start` (gaps[i] unused bytes ahead of packet i); `tail`
    unused bytes after the last one (0: it ends exactly at data_len). Bytes are random, so a wrong source shows."""
    lens = np.asarray(lens, dtype=np.uint32)
    g = np.zeros(len(lens), np.uint64) if gaps is None else np.asarray(gaps, dtype=np.uint64)
    step = lens.astype(np.uint64) + g
    offs = np.uint64(start) + np.cumsum(step) - lens.astype(np.uint64) if len(lens) else np.zeros(0, np.uint64)
    total = int(start + step.sum()) + tail
    data = np.random.default_rng(seed).integers(0, 256, total, dtype=np.uint8)
    return data, offs.astype(np.uint64), lens


def mix_lens(n: int, hi: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, hi + 1, n).astype(np.uint32)


def shuffled(c, seed: int):
    """The same packets with their descriptors in a random order (the rule's per-packet arrays stay as they are)."""
    perm = np.random.default_rng(seed).permutation(c.n)
    return replace(c, offsets=c.offsets[perm], caplens=c.caplens[perm])


def overlapped(c):
    """2n descriptors: every packet twice, the second one starting (up to 3 B) inside the first. The caller replaces the
    rule's per-packet arrays by ones of the new length."""
    twice = np.repeat(np.arange(c.n), 2)
    offs, lens = c.offsets[twice].copy(), c.caplens[twice].copy()
    offs[1::2] += np.minimum(lens[1::2], 3)
    lens[1::2] -= np.minimum(lens[1::2], 3)
    return replace(c, offsets=offs, caplens=lens)


def with_bad_descriptors(c):
    """Bad descriptors mixed in: past the end, a huge caplen, an offset whose end wraps 64 bits."""
    offs, lens = c.offsets.copy(), c.caplens.copy()
    offs[5::37] = len(c.data) - 1
    lens[5::37] = np.maximum(lens[5::37], 2)
    lens[11::53] = 0xFFFFFFF0
    offs[17::101] = np.uint64(0xFFFFFFFFFFFFFFF0)
    lens[17::101] = 64
    offs[64] = len(c.data)  # an empty packet at the very end is in bounds ...
    lens[64] = 0
    offs[65] = len(c.data)  # ... one byte there is not
    lens[65] = 1
    return replace(c, offsets=offs, caplens=lens)
