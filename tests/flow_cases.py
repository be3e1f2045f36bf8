"""The two flow tables at their edges: the model, crafted keys, guarded arenas and the checker (test helper for
test_flow_table.py).

The count table (pcppx_flow_count_device / _keys_device: flow_count_kernel + flow_merge_kernel) and the filter's table
(pcppx_filter_device: filter_mark_kernel + filter_apply_kernel) are open-addressed hash tables whose slot positions
depend on the order in which threads claim them, so a table is never compared slot by slot. What is compared:
  every stored key once, in the region of its partition, with exactly the counts of an integer group-by of the input;
  zero counts in every slot whose key is 0; stored + key-0 + lost packets = packets offered;
  every byte of the 4096-B guards around each array still the fill, the word behind stats[2] included.

The hash multipliers and shape constants of the kernels are restated here as plain numbers. They are used to aim the
inputs only (keys that share a home slot, a partition, a region slot; batches that cross a threshold): no expectation
is computed from them except "a key sits in the region of its partition", which pcppx.h states as the table's layout.
If the kernels' constants drift, the CPU tests of the aim still pass but the cases no longer reach their code paths;
the region check turns red if the partition constant or the region rule drifts.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

GUARD = 4096
FILL = 0x5A

# ------------------------------------------------------------------ the kernels' constants, restated
MUL_PART = 0x9E3779B1   # partition and count-LDS home: the top bits of key * MUL_PART; the filter's slot: its low bits
MUL_SLOT = 0x85EBCA6B   # region slot: the low bits of key * MUL_SLOT
MUL_MERGE = 0xC2B2AE35  # merge-LDS home: the top 12 bits of key * MUL_MERGE
MAX_PARTS = 512
MIN_REGION = 4096
BATCH = 6144            # packets per LDS batch of a count block
BLOCKS = 256            # persistent count blocks at most
COUNT_LDS = 8192        # slots of the count kernel's LDS table
MERGE_LDS = 4096        # slots of the merge kernel's LDS table
HOT = 2                 # a flow with more packets than this stays in LDS between batches ...
KEEP = COUNT_LDS // 2 - BATCH // 2  # ... while fewer than this many are kept (1024)
MERGE_ROUND = 1024      # queue records per merge round
MERGE_FLUSH = MERGE_LDS // 2  # the merge flushes its LDS table above this many used slots
LAUNCH_MAX = (1 << 24) - 1    # packets per launch (packets << 40 | bytes in one word)
MAX_CAPLEN = 65535
BYTES_BOUND = LAUNCH_MAX * MAX_CAPLEN  # one flow of a full launch: 2^40 - 2^24 - 2^16 + 1
assert BYTES_BOUND == (1 << 40) - (1 << 24) - (1 << 16) + 1 and BYTES_BOUND < 1 << 40
assert KEEP == 1024

_M32 = np.uint64(0xFFFFFFFF)


def _mul(keys, a: int) -> np.ndarray:
    return (np.asarray(keys).astype(np.uint64) * np.uint64(a)) & _M32


def _inv(a: int) -> int:
    return pow(a, -1, 1 << 32)


def _log2(v: int) -> int:
    assert v > 0 and v & (v - 1) == 0, v
    return v.bit_length() - 1


def partitions(capacity: int) -> int:
    """pcppx.h: min(512, max(1, capacity / 4096)) equal regions."""
    return min(MAX_PARTS, max(1, capacity // MIN_REGION))


def region_slots(capacity: int) -> int:
    return capacity // partitions(capacity)


def part_of(keys, capacity: int) -> np.ndarray:
    lp = _log2(partitions(capacity))
    x = _mul(keys, MUL_PART)
    return (x >> np.uint64(32 - lp)).astype(np.int64) if lp else np.zeros(len(x), np.int64)


def region_slot_of(keys, capacity: int) -> np.ndarray:
    return (_mul(keys, MUL_SLOT) & np.uint64(region_slots(capacity) - 1)).astype(np.int64)


def count_home_of(keys) -> np.ndarray:
    return (_mul(keys, MUL_PART) >> np.uint64(32 - _log2(COUNT_LDS))).astype(np.int64)


def merge_home_of(keys) -> np.ndarray:
    return (_mul(keys, MUL_MERGE) >> np.uint64(32 - _log2(MERGE_LDS))).astype(np.int64)


def filter_slot_of(hash5, capacity: int) -> np.ndarray:
    return (_mul(hash5, MUL_PART) & np.uint64(capacity - 1)).astype(np.int64)


def queue_capacity(n: int, capacity: int) -> int:
    """flow_queue_capacity: records per partition queue."""
    per = min(LAUNCH_MAX, n)
    parts = partitions(capacity)
    if parts == 1:
        return per
    even = (per + parts - 1) // parts
    return even + even // 4 + 4096


# ------------------------------------------------------------------ keys
def distinct(count: int, salt: int = 1) -> np.ndarray:
    """`count` distinct non-zero u32 keys (an odd multiplier is a bijection of the non-zero residues onto themselves)."""
    return _mul(np.arange(1, count + 1, dtype=np.uint64) + np.uint64(salt << 24), 0x2545F491).astype(np.uint32)


def craft(count: int, capacity: int | None = None, part: int | None = None, slot=None, count_home: int | None = None,
          merge_home: int | None = None) -> np.ndarray:
    """`count` distinct non-zero u32 keys with the prescribed partition (of a table of `capacity` slots), region slot
    (one value, or several taken in turn), count-LDS home and / or merge-LDS home. One property is solved with its
    multiplier's inverse mod 2^32 (all keys of a residue class or of a range of products), the others filter those
    candidates forward."""
    if slot is not None:
        r = _log2(region_slots(capacity))
        t = np.arange(1 << min(32 - r, 21), dtype=np.uint64) << np.uint64(r)
        # key * MUL_SLOT = s (mod 2^r)  <=>  key = s * MUL_SLOT^-1 (mod 2^r)
        res = [np.uint64((int(s) * _inv(MUL_SLOT)) & ((1 << r) - 1)) for s in np.atleast_1d(slot)]
        cand = np.stack([t + x for x in res], axis=1).reshape(-1)
    elif count_home is not None:
        b = 32 - _log2(COUNT_LDS)
        cand = _mul((np.uint64(count_home) << np.uint64(b)) | np.arange(1 << b, dtype=np.uint64), _inv(MUL_PART))
    elif part is not None:
        b = 32 - _log2(partitions(capacity))
        cand = _mul((np.uint64(part) << np.uint64(b)) | np.arange(1 << min(b, 22), dtype=np.uint64), _inv(MUL_PART))
    elif merge_home is not None:
        b = 32 - _log2(MERGE_LDS)
        cand = _mul((np.uint64(merge_home) << np.uint64(b)) | np.arange(1 << b, dtype=np.uint64), _inv(MUL_MERGE))
    else:
        return distinct(count)
    keep = cand != 0
    if part is not None:
        keep &= part_of(cand, capacity) == part
    if slot is not None:
        keep &= np.isin(region_slot_of(cand, capacity), np.atleast_1d(slot))
    if count_home is not None:
        keep &= count_home_of(cand) == count_home
    if merge_home is not None:
        keep &= merge_home_of(cand) == merge_home
    out = cand[keep][:count].astype(np.uint32)
    assert len(out) == count and len(np.unique(out)) == count, (len(out), count)
    return out


# ------------------------------------------------------------------ the expectation: an exact group-by
@dataclass
class Expect:
    keys: np.ndarray     # u32, sorted, distinct, non-zero
    packets: np.ndarray  # u64 per key
    bytes: np.ndarray    # u64 per key
    zero_packets: int    # key 0: stats[0]
    zero_bytes: int      # key 0: stats[1]
    n: int               # packets offered


def expected(keys, lens) -> Expect:
    """Packets and bytes per key of one call, in integer arithmetic (a stable sort and uint64 sums)."""
    keys = np.asarray(keys).astype(np.uint32)
    lens = np.asarray(lens).astype(np.uint64)
    assert keys.shape == lens.shape and keys.ndim == 1 and len(keys) > 0
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.concatenate(([True], ks[1:] != ks[:-1])))
    uniq = ks[starts]
    pk = np.diff(np.concatenate((starts, [len(ks)]))).astype(np.uint64)
    by = np.add.reduceat(lens[order], starts).astype(np.uint64)
    z = int(uniq[0] == 0)
    return Expect(uniq[z:], pk[z:], by[z:], int(pk[0]) if z else 0, int(by[0]) if z else 0, len(keys))


def one_flow(key: int, n: int, length: int) -> Expect:
    """n packets of one non-zero key and one length: the analytic expectation."""
    return Expect(np.array([key], np.uint32), np.array([n], np.uint64), np.array([n * length], np.uint64), 0, 0, n)


# ------------------------------------------------------------------ images: name -> u8[GUARD + size + GUARD]
TABLE_DTYPES = {"keys": np.uint32, "packets": np.uint64, "bytes": np.uint64, "stats": np.uint64}


def table_sizes(capacity: int) -> dict[str, int]:
    return {"keys": 4 * capacity, "packets": 8 * capacity, "bytes": 8 * capacity, "stats": 3 * 8}


def blank_image(sizes: dict[str, int]) -> dict[str, np.ndarray]:
    """Arenas on the host: guards of FILL, zeroed payloads."""
    img = {}
    for name, size in sizes.items():
        a = np.full(2 * GUARD + size, FILL, np.uint8)
        a[GUARD:GUARD + size] = 0
        img[name] = a
    return img


def payload(img: dict, name: str, dtype=None) -> np.ndarray:
    a = img[name]
    return a[GUARD:len(a) - GUARD].view(dtype or TABLE_DTYPES[name])


class Arena:
    """The arenas of one table on the device: keys, packets, bytes, stats (3 words) and any input column, each alone
    between two GUARD-byte guards of FILL; table payloads zeroed, input payloads loaded."""

    def __init__(self, capacity: int, device: str = "cuda:0", sizes: dict | None = None, **inputs):
        import torch

        self.capacity = capacity
        self.t = {}
        self.inputs = {k: np.ascontiguousarray(v) for k, v in inputs.items()}
        sizes = dict(table_sizes(capacity) if sizes is None else sizes)
        sizes.update({k: max(v.nbytes, 8) for k, v in self.inputs.items()})
        for name, size in sizes.items():
            t = torch.full((2 * GUARD + size,), FILL, dtype=torch.uint8, device=device)
            assert t.data_ptr() % 256 == 0
            if name in self.inputs:
                raw = self.inputs[name].view(np.uint8).reshape(-1)
                t[GUARD:GUARD + len(raw)] = torch.from_numpy(raw).to(device)
            else:
                t[GUARD:GUARD + size] = 0
            self.t[name] = t

    def out(self, name: str):
        """The tensor handed to the library (arena + GUARD)."""
        t = self.t[name]
        return t[GUARD:t.numel() - GUARD]

    def host(self) -> dict[str, np.ndarray]:
        return {name: t.cpu().numpy() for name, t in self.t.items()}


# ------------------------------------------------------------------ the checker
class FlowTableError(AssertionError):
    """A table image breaks one of the rules; `kind` names it."""

    def __init__(self, kind: str, msg: str):
        super().__init__(f"{kind}: {msg}")
        self.kind = kind


@dataclass
class Checked:
    keys: np.ndarray     # the stored keys, in slot order
    slots: np.ndarray    # their slots
    missing: np.ndarray  # keys of the input that are not stored
    lost: int            # stats[2]


def check_guards(img: dict, inputs: dict | None = None) -> None:
    """Every arena's guards still FILL (the word behind stats[2] named apart), every input column unchanged."""
    inputs = inputs or {}
    for name, a in img.items():
        front, rear = a[:GUARD], a[len(a) - GUARD:]
        if name == "stats" and (rear[:8] != FILL).any():
            raise FlowTableError("stats[3]", f"the word behind stats[2] holds {rear[:8].view(np.uint64)[0]:#x}: stats is "
                                             "three words")
        for side, g in (("front", front), ("rear", rear)):
            bad = np.flatnonzero(g != FILL)
            if len(bad):
                raise FlowTableError("guard", f"{name}: {len(bad)} bytes of the {side} guard touched, first at guard byte "
                                              f"{int(bad[0])} (holds {int(g[bad[0]]):#04x})")
        if name in inputs:
            raw = np.ascontiguousarray(inputs[name]).view(np.uint8).reshape(-1)
            if not np.array_equal(a[GUARD:GUARD + len(raw)], raw):
                raise FlowTableError("input changed", f"{name}: an input column was written")


def check_table(img: dict, capacity: int, exp: Expect, calls: int = 1, lost_ok: bool = False,
                inputs: dict | None = None) -> Checked:
    """A count table's image after `calls` identical calls (or one call of the concatenated input) against the group-by.
    lost_ok: stats[2] may be non-zero, and then every region that lost a key must be full. Raises FlowTableError."""
    check_guards(img, inputs)
    keys, pk, by, stats = (payload(img, x) for x in ("keys", "packets", "bytes", "stats"))
    assert len(keys) == len(pk) == len(by) == capacity and len(stats) == 3
    used = keys != 0
    slots = np.flatnonzero(used)
    k = keys[slots]
    uk, cnt = np.unique(k, return_counts=True)
    if len(uk) != len(k):
        twice = int(uk[cnt > 1][0])
        raise FlowTableError("duplicate key", f"key {twice:#x} is stored in slots {np.flatnonzero(keys == twice).tolist()}")
    rs = region_slots(capacity)
    off = np.flatnonzero(slots // rs != part_of(k, capacity))
    if len(off):
        i = int(off[0])
        raise FlowTableError("wrong region", f"key {int(k[i]):#x} sits in slot {int(slots[i])} (region {int(slots[i]) // rs}"
                                             f" of {partitions(capacity)}), its partition is "
                                             f"{int(part_of(k[i:i + 1], capacity)[0])}: a key outside its own region -- or "
                                             f"the partition constant {MUL_PART:#x} / the region rule restated in "
                                             "flow_cases.py is no longer the kernels'")
    stray = np.flatnonzero(~used & ((pk != 0) | (by != 0)))
    if len(stray):
        s = int(stray[0])
        raise FlowTableError("empty slot count", f"slot {s} has key 0 and counts ({int(pk[s])}, {int(by[s])})")
    idx = np.minimum(np.searchsorted(exp.keys, k), max(len(exp.keys) - 1, 0))
    known = exp.keys[idx] == k if len(exp.keys) else np.zeros(len(k), bool)
    if not known.all():
        i = int(np.flatnonzero(~known)[0])
        raise FlowTableError("unknown key", f"slot {int(slots[i])} holds key {int(k[i]):#x}, which no packet has")
    c = np.uint64(calls)
    wpk, wby = exp.packets[idx] * c, exp.bytes[idx] * c
    bad = np.flatnonzero((pk[slots] != wpk) | (by[slots] != wby))
    if len(bad):
        i = int(bad[0])
        s = int(slots[i])
        dpk, dby = int(pk[s]) - int(wpk[i]), int(by[s]) - int(wby[i])
        kind = "carry" if dpk != 0 and (dby + (dpk << 40)) % (1 << 64) == 0 else "wrong count"
        raise FlowTableError(kind, f"{len(bad)} keys, first {int(k[i]):#x} in slot {s}: ({int(pk[s])}, {int(by[s])}), "
                                   f"expected ({int(wpk[i])}, {int(wby[i])})")
    if (int(stats[0]), int(stats[1])) != (exp.zero_packets * calls, exp.zero_bytes * calls):
        raise FlowTableError("key 0", f"stats[0:2] = ({int(stats[0])}, {int(stats[1])}), expected "
                                      f"({exp.zero_packets * calls}, {exp.zero_bytes * calls})")
    stored = int(pk[slots].sum())
    if stored + int(stats[0]) + int(stats[2]) != exp.n * calls:
        raise FlowTableError("conservation", f"stored {stored} + key-0 {int(stats[0])} + lost {int(stats[2])} != "
                                             f"{exp.n * calls} packets offered")
    missing = np.setdiff1d(exp.keys, k)
    if not lost_ok:
        if int(stats[2]) != 0 or len(missing):
            raise FlowTableError("lost", f"stats[2] = {int(stats[2])}, {len(missing)} keys missing: nothing may be lost here")
    else:
        for p in np.unique(part_of(missing, capacity)).tolist():
            free = np.flatnonzero(~used[p * rs:(p + 1) * rs])
            if len(free):
                raise FlowTableError("lost with room", f"region {p} lost a key and has {len(free)} empty slots")
    return Checked(k, slots, missing, int(stats[2]))


def as_dict(img: dict) -> dict:
    """{key: (packets, bytes)} of an image that passed check_table (no key twice), and its stats."""
    keys, pk, by = (payload(img, x) for x in ("keys", "packets", "bytes"))
    s = np.flatnonzero(keys)
    return dict(zip(keys[s].tolist(), zip(pk[s].tolist(), by[s].tolist()))), payload(img, "stats").tolist()


# ------------------------------------------------------------------ the numpy stand-in
def model_image(capacity: int, keys_in, lens_in, calls: int = 1) -> dict[str, np.ndarray]:
    """A correct table built from the model: every distinct key, in order of first appearance, probes linearly from
    its region slot inside the region of its partition; a key whose region is full is counted in stats[2]."""
    exp = expected(keys_in, lens_in)
    img = blank_image(table_sizes(capacity))
    keys, pk, by, stats = (payload(img, x) for x in ("keys", "packets", "bytes", "stats"))
    rs = region_slots(capacity)
    k_in = np.asarray(keys_in).astype(np.uint32)
    _, first = np.unique(k_in, return_index=True)
    order = k_in[np.sort(first)]
    order = order[order != 0]
    where = np.searchsorted(exp.keys, order)
    parts, homes = part_of(order, capacity), region_slot_of(order, capacity)
    for key, w, p, h in zip(order.tolist(), where.tolist(), parts.tolist(), homes.tolist()):
        for probe in range(rs):
            s = p * rs + (h + probe) % rs
            if keys[s] == 0:
                keys[s] = key
                pk[s] = exp.packets[w] * np.uint64(calls)
                by[s] = exp.bytes[w] * np.uint64(calls)
                break
        else:
            stats[2] += exp.packets[w] * np.uint64(calls)
    stats[0], stats[1] = exp.zero_packets * calls, exp.zero_bytes * calls
    return img


# ------------------------------------------------------------------ the input columns of the GPU cases
def lengths(n: int, seed: int, edges: bool = True) -> np.ndarray:
    """n lengths of 60 to 1514; with `edges` one packet of length 0 and one of 65535 (n == 1: 65535 alone)."""
    lens = np.random.default_rng(seed).integers(60, 1515, n).astype(np.uint32)
    if edges:
        lens[n // 2] = 0
        lens[n - 1] = MAX_CAPLEN
    return lens


N_EDGES = (1, 63, 64, 65, 1023, 1024, 1025, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH - 1, 2 * BATCH + 1,
           BLOCKS * BATCH - 1, BLOCKS * BATCH, BLOCKS * BATCH + 1, (BLOCKS + 1) * BATCH + 1)
COLUMNS = ("distinct", "one", "zero")
SUMMARY_TOO = ((1, "distinct"), (1025, "distinct"), (BATCH + 1, "one"), (BLOCKS * BATCH + 1, "distinct"),
               ((BLOCKS + 1) * BATCH + 1, "zero"))


def n_edge_table() -> list[tuple[int, str, int]]:
    """(n, column, capacity): every n with every column; every n and every column with both capacities (4096 only
    where the distinct keys fit one region)."""
    rows = []
    for i, n in enumerate(N_EDGES):
        small = n <= 4096
        rows.append((n, "distinct", 4096 if small else 1 << 21))
        rows.append((n, "one", 1 << 21 if small else 4096))
        rows.append((n, "zero", 4096 if i % 2 else 1 << 21))
    return rows


def n_edge_keys(n: int, column: str) -> np.ndarray:
    if column == "distinct":
        return distinct(n, salt=3)
    return np.full(n, 0x1234567 if column == "one" else 0, np.uint32)


def ladder_flows(capacity: int) -> int:
    return max(1, min(capacity // 2, 50_000))


LADDER = (1, 2, 4, 64, 4096, 8192, 1 << 14, 1 << 20, 1 << 21, 1 << 22)


def ladder_keys(capacity: int) -> np.ndarray:
    """4 * flows + 1 packets over `flows` distinct keys, shuffled."""
    flows = ladder_flows(capacity)
    pool = distinct(flows, salt=5)
    n = 4 * flows + 1
    return pool[np.random.default_rng(capacity).permutation(n) % flows]


def cycle(pool: np.ndarray, n: int) -> np.ndarray:
    return pool[np.arange(n) % len(pool)]


HOT_N = 2 * BLOCKS * BATCH + 17
HOT_COLUMNS = ("quads", "zipf", "threshold")


def hot_keys(column: str) -> np.ndarray:
    """quads: packet i belongs to flow (i % 6144) // 4 -- 1536 flows of 4 packets in every batch, all hot, more than the
    1024 a block keeps. zipf: Zipf(1.1) over 100k flows. threshold: per batch one flow of exactly 2 packets, one of
    exactly 3 (either side of "more than 2"), every other packet a flow of its own position."""
    i = np.arange(HOT_N, dtype=np.int64)
    if column == "quads":
        return distinct(BATCH // 4, salt=7)[(i % BATCH) // 4]
    if column == "zipf":
        ranks = np.minimum(np.random.default_rng(11).zipf(1.1, HOT_N), 100_000)
        return distinct(100_000, salt=8)[ranks - 1]
    pos = i % BATCH
    pool = distinct(BATCH, salt=9)
    return pool[np.where(pos < 2, 0, np.where(pos < 5, 2, pos))]


def block_batches(n: int):
    """(block, start, end) of every batch of a launch of n <= LAUNCH_MAX packets, as the count kernel walks them."""
    grid = min(BLOCKS, -(-n // BATCH))
    for base in range(0, n, BATCH):
        yield (base // BATCH) % grid, base, min(base + BATCH, n)


SPLIT_NS = (LAUNCH_MAX, LAUNCH_MAX + 1, LAUNCH_MAX + 1 + BATCH + 1)
SPLIT_KEY = 0x0BADCAFE


def split_column2(n: int) -> tuple[np.ndarray, np.ndarray]:
    i = np.arange(n, dtype=np.uint32)
    return i % np.uint32(100003) + np.uint32(1), np.uint32(60) + i % np.uint32(1455)


# ------------------------------------------------------------------ the filter's table
def filter_slot_keys(count: int, capacity: int, slot: int) -> np.ndarray:
    """`count` distinct non-zero hash5 values whose filter slot, (hash5 * MUL_PART) & (capacity - 1), is `slot`."""
    b = _log2(capacity)
    t = np.arange(1, count + 2, dtype=np.uint64) << np.uint64(b)
    cand = (t + np.uint64((slot * _inv(MUL_PART)) & (capacity - 1))) & _M32
    out = cand[cand != 0][:count].astype(np.uint32)
    assert len(np.unique(out)) == count and (filter_slot_of(out, capacity) == slot).all()
    return out


FILTER_ML = 8
SP, DP = 40000, 50000
UF, UR, TF, TR, ARP, V6 = range(6)  # UDP / TCP forward (source port SP) and reverse, ARP, IPv6 UDP


@lru_cache(maxsize=None)
def filter_kinds():
    """The six packets every filter case is made of, and the restatement's records of them at max_layers 8."""
    import mutate
    import oracle
    from pcapplusplus_amd import abi

    e4 = mutate._eth(0x0800)
    pk = [e4 + mutate._ipv4(17, 12) + mutate._udp(SP, DP, b"flow"), e4 + mutate._ipv4(17, 12) + mutate._udp(DP, SP, b"back"),
          e4 + mutate._ipv4(6, 24) + mutate._tcp(SP, DP, b"flow"), e4 + mutate._ipv4(6, 24) + mutate._tcp(DP, SP, b"back"),
          mutate._eth(0x0806) + bytes(28), mutate._eth(0x86DD) + mutate._ipv6(17, 12) + mutate._udp(DP, SP, b"six!")]
    b = mutate.as_batch(pk)
    s, lay = oracle.oracle_parse(b, abi.make_opts(0, 8, False, FILTER_ML))
    assert s["hash5"][ARP] == 0 and (s["hash5"][[UF, UR, TF, TR, V6]] != 0).all()
    return b, s, lay


@dataclass
class FilterCase:
    batch: object        # PacketBatch: descriptors into the six packets' bytes
    summary: np.ndarray  # the restatement's records, hash5 overwritten with the chosen flow keys
    layers: np.ndarray   # [n, FILTER_ML]
    kinds: np.ndarray
    hash5: np.ndarray


def filter_case(kinds, hash5) -> FilterCase:
    from pcapplusplus_amd.pcap import PacketBatch

    kb, s, lay = filter_kinds()
    kinds = np.asarray(kinds, np.int64)
    hash5 = np.asarray(hash5).astype(np.uint32)
    assert kinds.shape == hash5.shape
    summary = s[kinds].copy()
    summary["hash5"] = hash5
    batch = PacketBatch(kb.data, kb.offsets[kinds].copy(), kb.caplens[kinds].copy(), kb.linktype)
    return FilterCase(batch, summary, np.ascontiguousarray(lay[kinds]), kinds, hash5)


def filter_own(case: FilterCase, spec) -> np.ndarray:
    """Per packet: does it match the spec on its own (the restatement over the six kinds, every one a flow of its
    own)."""
    import oracle

    kb, s, lay = filter_kinds()
    s = s.copy()
    s["hash5"] = np.arange(1, len(s) + 1)
    own, _ = oracle.oracle_filter(kb, s, lay, spec)
    return own[case.kinds].astype(bool)


def filter_expect(case: FilterCase, spec, seq_base: int = 0):
    """(matched, stats, {1 << 32 | hash5: sequence number of the flow's first own-matching packet}): the restatement's
    verdicts and counters over the edited records; its flow table keeps no sequence numbers, so `first` comes from the
    own-matching packets."""
    import oracle

    matched, stats = oracle.oracle_filter(case.batch, case.summary, case.layers, spec)
    stats["flow_table_full"] = 0
    own = filter_own(case, spec)
    table = {}
    for i in np.flatnonzero(own).tolist():
        table.setdefault((1 << 32) | int(case.hash5[i]), seq_base + i)
    return matched, stats, table


FILTER_STATS_WORDS = 15  # sizeof(pcppx_packet_stats) / 8


def run_filter(engine, case: FilterCase, spec, capacity: int, cuts=(), seq_base: int = 0, device: str = "cuda:0") -> dict:
    """pcppx_filter_device over the case's records in consecutive calls cut at `cuts`, every output in a guarded
    arena; returns the image."""
    import torch

    from pcapplusplus_amd.engine import to_device

    n = case.batch.n
    data, offsets, caplens = to_device(case.batch, device)
    summ = torch.from_numpy(case.summary.view(np.uint8).reshape(-1).copy()).to(device)
    lay = torch.from_numpy(case.layers.view(np.uint8).reshape(-1).copy()).to(device)
    ar = Arena(capacity, device, sizes={"matched": n, "flow_keys": 8 * capacity, "flow_first": 8 * capacity,
                                         "pstats": 8 * FILTER_STATS_WORDS})
    st = torch.cuda.current_stream(device).cuda_stream
    bounds = [0, *cuts, n]
    for a, z in zip(bounds[:-1], bounds[1:]):
        engine.filter_device(data, offsets[a:z], caplens[a:z], z - a, case.batch.linktype, summ[a * 32:z * 32],
                             lay[a * FILTER_ML * 8:z * FILTER_ML * 8], FILTER_ML, spec, seq_base + a,
                             ar.out("flow_keys"), ar.out("flow_first"), capacity, ar.out("matched")[a:z],
                             ar.out("pstats"), st)
    torch.cuda.synchronize(device)
    return ar.host()


def filter_table(img: dict, capacity: int) -> dict:
    """{flow key: first sequence number} of a filter image: guards untouched, no key twice, every used key of the form
    1 << 32 | hash5, flow_first 0 wherever flow_keys is 0."""
    check_guards(img)
    keys, first = payload(img, "flow_keys", np.uint64), payload(img, "flow_first", np.uint64)
    assert len(keys) == len(first) == capacity
    used = keys != 0
    if len(np.unique(keys[used])) != int(used.sum()):
        raise FlowTableError("duplicate key", f"flow_keys holds a key twice: {keys[used].tolist()}")
    if ((keys[used] >> np.uint64(32)) != 1).any():
        raise FlowTableError("unknown key", f"a used flow_keys slot is not 1 << 32 | hash5: {keys[used].tolist()}")
    if (first[~used] != 0).any():
        raise FlowTableError("empty slot count", "flow_first is non-zero in a slot whose key is 0")
    return {int(k): int(~f & np.uint64(0xFFFFFFFFFFFFFFFF)) for k, f in zip(keys[used], first[used])}


def filter_stats(img: dict) -> dict:
    from pcapplusplus_amd import abi

    return {k: int(v) for k, v in zip(abi.STATS_FIELDS, payload(img, "pstats", np.uint64))}
