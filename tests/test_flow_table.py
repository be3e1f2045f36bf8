"""The flow-count table (flow_count_kernel + flow_merge_kernel) and the filter's flow table (filter_mark_kernel +
filter_apply_kernel) at their edges: guarded arenas, crafted keys, an exact integer group-by (flow_cases.py).

CPU: the model restates pcppx.h's layout; craft() gives keys with the prescribed homes (recomputed forward for every
set the GPU cases use); every GPU case's input reaches the code path it is aimed at, by the model; the checker passes
a correct table built by a numpy stand-in and fails, by `kind`, on each injected fault; pcppx.h states the limits the
cases rely on.
GPU: every case runs through flow_cases.Arena and check_table -- no tolerance anywhere, every count exact.

The launch-split cases (n >= 2^24 - 1) are the one place where the smallest shape that can fail is large: 16.8M packets,
134 MB of input columns per case. Measured on an MI355X: 0.1 s per one-flow case and 0.4 s per many-flows case, the
host group-by included, so both columns run at all three n.
"""
from __future__ import annotations

import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import flow_cases as fc
import oracle
from flow_cases import BATCH, BLOCKS, FlowTableError
from pcapplusplus_amd import abi

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------ the crafted sets the GPU cases use
@lru_cache(maxsize=None)
def full_region_keys(capacity: int, extra: int) -> np.ndarray:
    """capacity + extra distinct keys for a one-region table."""
    return fc.distinct(capacity + extra, salt=13)


@lru_cache(maxsize=None)
def two_region_keys(extra: int) -> tuple[np.ndarray, np.ndarray]:
    """Capacity 8192: 4096 + extra keys of partition 1 (a full region), 10 keys of partition 0."""
    return fc.craft(4096 + extra, 8192, part=1), fc.craft(10, 8192, part=0)


@lru_cache(maxsize=None)
def wrap_keys() -> tuple[np.ndarray, np.ndarray]:
    """Capacity 2^21: 600 keys of the last partition with region slot 4095, 600 of partition 0 with 4094 / 4095."""
    return fc.craft(600, 1 << 21, part=511, slot=4095), fc.craft(600, 1 << 21, part=0, slot=(4094, 4095))


@lru_cache(maxsize=None)
def count_lds_keys() -> np.ndarray:
    return fc.craft(4000, count_home=fc.COUNT_LDS - 1)


@lru_cache(maxsize=None)
def merge_lds_keys() -> np.ndarray:
    return fc.craft(3000, merge_home=fc.MERGE_LDS - 1)


# ------------------------------------------------------------------ CPU: the model and the aim
def test_model_restates_the_header_layout():
    """pcppx.h: min(512, max(1, capacity / 4096)) equal regions; the region rule changes at 4096 -> 8192 (1 -> 2
    regions) and at 2^21 -> 2^22 (512 regions of 4096 -> of 8192 slots)."""
    text = (ROOT / "include" / "pcppx.h").read_text()
    assert "min(512, max(1, capacity / 4096)) equal regions" in text
    want = {1: (1, 1), 2: (1, 2), 4: (1, 4), 64: (1, 64), 4096: (1, 4096), 8192: (2, 4096), 1 << 14: (4, 4096),
            1 << 20: (256, 4096), 1 << 21: (512, 4096), 1 << 22: (512, 8192)}
    assert set(want) == set(fc.LADDER)
    for cap, (parts, slots) in want.items():
        assert (fc.partitions(cap), fc.region_slots(cap)) == (parts, slots), cap
    assert fc.queue_capacity(10, 4096) == 10 and fc.queue_capacity(1 << 25, 4096) == fc.LAUNCH_MAX
    assert fc.queue_capacity(3_000_000, 1 << 21) == 5860 + 1465 + 4096


def test_header_states_the_limits():
    """The sentences of pcppx.h the cases rely on: the caplen bound under non-zero keys, three stats words, zero counts
    under key 0, the launch split, and the one sequence number the filter's ~seq cannot hold."""
    text = re.sub(r"\s*\n\s*\*\s*", " ", (ROOT / "include" / "pcppx.h").read_text())
    for sentence in ("caplens[i] <= PCPPX_MAX_CAPLEN is required wherever the key is non-zero",
                     "OVERSIZE and BAD_DESC packets have key 0",
                     "With larger values the per-flow counts are unspecified",
                     "stats is three words",
                     "Slots with key 0 keep zero counts",
                     "A call of more than 2^24 - 1 packets is processed in consecutive launches with the same result",
                     "seq_base + n must stay below 2^64 - 1"):
        assert sentence in text, sentence


def test_craft_properties_forward():
    """Every crafted set of the GPU cases, recomputed forward: distinct, non-zero, the prescribed homes."""
    for extra in (0, 1):
        p1, p0 = two_region_keys(extra)
        assert len(p1) == 4096 + extra and (fc.part_of(p1, 8192) == 1).all() and (fc.part_of(p0, 8192) == 0).all()
        assert len(np.unique(np.concatenate([p1, p0]))) == len(p1) + 10 and p1.all() and p0.all()
    last, first = wrap_keys()
    assert (fc.part_of(last, 1 << 21) == 511).all() and (fc.region_slot_of(last, 1 << 21) == 4095).all()
    assert (fc.part_of(first, 1 << 21) == 0).all()
    assert sorted(np.unique(fc.region_slot_of(first, 1 << 21)).tolist()) == [4094, 4095]
    assert len(np.unique(np.concatenate([last, first]))) == 1200 and last.all() and first.all()
    c = count_lds_keys()
    assert len(np.unique(c)) == 4000 and c.all() and (fc.count_home_of(c) == 8191).all()
    m = merge_lds_keys()
    assert len(np.unique(m)) == 3000 and m.all() and (fc.merge_home_of(m) == 4095).all()
    for cap, slot, count in ((64, 63, 40), (8, 7, 8), (1, 0, 2), (2, 1, 3)):
        h = fc.filter_slot_keys(count, cap, slot)
        assert len(np.unique(h)) == count and h.all() and (fc.filter_slot_of(h, cap) == slot).all()
    # the multipliers' inverses really invert
    for a in (fc.MUL_PART, fc.MUL_SLOT, fc.MUL_MERGE):
        assert (a * fc._inv(a)) % (1 << 32) == 1
    d = fc.distinct(1 << 20)
    assert len(np.unique(d)) == 1 << 20 and d.all()


def test_expected_is_an_exact_group_by():
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 50, 5000).astype(np.uint32)
    lens = rng.integers(0, 1 << 32, 5000).astype(np.uint64)  # sums far past 2^53: exact only in integers
    e = fc.expected(keys, lens)
    want: dict = {}
    for k, ln in zip(keys.tolist(), lens.tolist()):
        p, b = want.get(k, (0, 0))
        want[k] = (p + 1, b + ln)
    zero = want.pop(0)
    assert dict(zip(e.keys.tolist(), zip(e.packets.tolist(), e.bytes.tolist()))) == want
    assert (e.zero_packets, e.zero_bytes, e.n) == (*zero, 5000)
    big = fc.expected(np.full(3, 7, np.uint32), np.full(3, (1 << 53) + 1, np.uint64))
    assert int(big.bytes[0]) == 3 * ((1 << 53) + 1)
    o = fc.one_flow(9, fc.LAUNCH_MAX, fc.MAX_CAPLEN)
    assert int(o.bytes[0]) == (1 << 40) - (1 << 24) - (1 << 16) + 1 == fc.BYTES_BOUND


def test_n_edge_table_is_pairwise():
    """Every n with every column; every n and every column with both capacities; 4096 only where the keys fit."""
    rows = fc.n_edge_table()
    assert len(rows) == len(set(rows)) <= 60
    assert {(n, c) for n, c, _ in rows} == {(n, c) for n in fc.N_EDGES for c in fc.COLUMNS}
    for n in fc.N_EDGES:
        assert {cap for m, _, cap in rows if m == n} == {4096, 1 << 21}, n
    for c in fc.COLUMNS:
        assert {cap for _, col, cap in rows if col == c} == {4096, 1 << 21}, c
    assert all(cap != 4096 or col != "distinct" or n <= 4096 for n, col, cap in rows)
    assert set(fc.SUMMARY_TOO) <= {(n, c) for n, c, _ in rows}
    assert fc.N_EDGES == (1, 63, 64, 65, 1023, 1024, 1025, 6143, 6144, 6145, 12287, 12289, 256 * 6144 - 1, 256 * 6144,
                          256 * 6144 + 1, 257 * 6144 + 1)
    lens = fc.lengths(1025, 1)
    assert (lens == 0).sum() == 1 and (lens == 65535).sum() == 1 and fc.lengths(1, 1).tolist() == [65535]


def test_ladder_and_full_region_inputs_reach_their_paths():
    for cap in fc.LADDER:
        k = fc.ladder_keys(cap)
        flows = fc.ladder_flows(cap)
        assert len(k) == 4 * flows + 1 and len(np.unique(k)) == flows == max(1, min(cap // 2, 50_000))
    for cap in (1, 2, 64, 4096):
        assert fc.partitions(cap) == 1
        for extra in (0, 1):
            k = fc.cycle(full_region_keys(cap, extra), 3 * (cap + extra))
            assert len(np.unique(k)) == cap + extra and k.all()
    for extra in (0, 1):
        p1, _ = two_region_keys(extra)
        assert len(p1) == fc.region_slots(8192) + extra  # one region's worth, or one more, in one region


def test_wrap_inputs_wrap_in_the_model():
    """The model puts each chain across its region's end: the run holds slot 4095 and slot 0 of its region."""
    last, first = wrap_keys()
    keys = np.concatenate([last, first])
    img = fc.model_image(1 << 21, keys, np.full(len(keys), 60))
    got = fc.check_table(img, 1 << 21, fc.expected(keys, np.full(len(keys), 60)))
    for p in (511, 0):
        assert_wrapped_run(got, 1 << 21, p, 600)


def test_overflow_wrap_input_overflows_its_queue():
    last, _ = wrap_keys()
    keys = fc.cycle(last, 8 * BATCH)
    records = sum(len(np.unique(keys[a:z])) for _, a, z in fc.block_batches(8 * BATCH))
    assert records == 4800 > fc.queue_capacity(8 * BATCH, 1 << 21) == 4216


def assert_wrapped_run(got: fc.Checked, capacity: int, part: int, count: int):
    """The occupied slots of region `part` are one contiguous run modulo the region size that holds the region's last
    slot and its first: the chain wrapped inside its region."""
    rs = fc.region_slots(capacity)
    occ = got.slots[(got.slots // rs) == part] - part * rs
    assert len(occ) == count
    here = np.zeros(rs, bool)
    here[occ] = True
    assert int((here & ~np.roll(here, -1)).sum()) == 1, "not one contiguous run"
    assert here[rs - 1] and here[0], "the run does not cross the region's end"


def test_lds_collision_inputs_reach_their_paths():
    """Count LDS: 4000 keys of one home in one 6144-packet batch -- one chain from slot 8191 around to slot 0. Merge
    LDS: every one of 4 blocks queues all 3000 keys, so the queue holds 12000 records of 3000 keys, the merge's LDS
    table passes 2048 used slots mid-queue and flushes while records of flushed keys are still to come."""
    k = fc.cycle(count_lds_keys(), BATCH)
    assert len(np.unique(k)) == 4000 and len(list(fc.block_batches(BATCH))) == 1
    assert len(list(fc.block_batches(3 * BATCH))) == 3
    k = fc.cycle(merge_lds_keys(), 4 * BATCH)
    records = [len(np.unique(k[a:z])) for _, a, z in fc.block_batches(4 * BATCH)]
    assert records == [3000] * 4 and sum(records) > 3000 > fc.MERGE_FLUSH
    assert fc.queue_capacity(4 * BATCH, 4096) >= sum(records)  # all through the queue, none by the atomic path
    # the first flush happens before the queue's end: 2048 distinct keys are met within the first 3 rounds of 1024
    assert fc.MERGE_FLUSH + fc.MERGE_ROUND < sum(records)


def test_hot_columns_cross_the_keep_limit_and_the_threshold():
    assert fc.HOT_N == 2 * 256 * 6144 + 17 > BLOCKS * BATCH  # every block sees a second batch
    q = fc.hot_keys("quads")
    t = fc.hot_keys("threshold")
    seen = 0
    for _, a, z in fc.block_batches(fc.HOT_N):
        if z - a < BATCH or seen >= 3 * BLOCKS // 2:
            continue
        seen += 1
        _, c = np.unique(q[a:z], return_counts=True)
        assert int((c > fc.HOT).sum()) == 1536 > fc.KEEP  # more hot flows than a block keeps
        _, c = np.unique(t[a:z], return_counts=True)
        assert sorted(c.tolist())[-3:] == [1, 2, 3]  # one flow on each side of "more than 2"
    z = fc.hot_keys("zipf")
    _, c = np.unique(z[:BATCH], return_counts=True)
    assert (c > fc.HOT).any() and len(np.unique(z)) > 20_000


def test_split_inputs_exceed_one_launch():
    assert fc.SPLIT_NS == ((1 << 24) - 1, 1 << 24, (1 << 24) + 6145)
    assert fc.SPLIT_NS[0] == fc.LAUNCH_MAX and all(n > fc.LAUNCH_MAX for n in fc.SPLIT_NS[1:])
    assert fc.SPLIT_NS[2] - fc.LAUNCH_MAX > BATCH  # the second launch has more than one batch
    k, ln = fc.split_column2(1000)
    assert k.min() == 1 and ln.min() == 60 and k.dtype == ln.dtype == np.uint32
    assert 60 + 1454 == 1514


@lru_cache(maxsize=None)
def oversize_batch():
    """footprint_cases' mixed batch (it holds the 70000-B OVERSIZE descriptor and the descriptors past data_len) plus
    three descriptors of caplen 65536, 70000 and 0xFFFFFFFF at offset 0; the restatement's records of it."""
    import footprint_cases as fp
    from pcapplusplus_amd.pcap import PacketBatch

    base = fp.batch(129, "unparsed")
    assert len(base.data) > fp.OVERSIZE
    offs = np.concatenate([base.offsets, np.zeros(3, np.uint64)])
    caps = np.concatenate([base.caplens, np.array([65536, 70000, 0xFFFFFFFF], np.uint32)])
    b = PacketBatch(base.data, offs, caps)
    opts = abi.make_opts(0, 8, False, 0)
    s, _ = oracle.oracle_parse(b, opts)
    return b, s, caps > abi.MAX_CAPLEN, opts


def test_oversize_and_bad_descriptors_have_key_zero():
    """The restatement: caplen > PCPPX_MAX_CAPLEN is OVERSIZE (or BAD_DESC where it passes data_len), key 0."""
    b, s, big, _ = oversize_batch()
    assert int(big.sum()) >= 4 and ((s["flags"][big] & (abi.F_OVERSIZE | abi.F_BAD_DESC)) != 0).all()
    assert [int(f) & (abi.F_OVERSIZE | abi.F_BAD_DESC) for f in s["flags"][-3:]] == [abi.F_OVERSIZE, abi.F_OVERSIZE,
                                                                                      abi.F_BAD_DESC]
    bad = (s["flags"] & abi.F_BAD_DESC) != 0
    assert int((bad & ~big).sum()) >= 1  # a past-data_len descriptor of ordinary length
    assert (s["hash5"][big | bad] == 0).all() and s["hash5"].any()
    assert fc.expected(s["hash5"], b.caplens).zero_bytes > 1 << 32


# ------------------------------------------------------------------ CPU: the checker on the stand-in
@lru_cache(maxsize=None)
def standin():
    """A 2-region table from the model: 300 keys, key-0 packets, two calls."""
    rng = np.random.default_rng(1)
    pool = np.concatenate([[0], fc.distinct(300, salt=21)]).astype(np.uint32)
    keys = pool[rng.integers(0, len(pool), 5000)]
    lens = fc.lengths(5000, 2)
    return keys, lens, fc.expected(keys, lens)


def fresh():
    keys, lens, exp = standin()
    return fc.model_image(8192, keys, lens, calls=2), exp


def test_checker_passes_the_standin():
    img, exp = fresh()
    got = fc.check_table(img, 8192, exp, calls=2)
    assert len(got.keys) == 300 and got.lost == 0 and len(got.missing) == 0
    # and a full one-region table that loses exactly one key
    keys = fc.cycle(full_region_keys(64, 1), 3 * 65)
    lens = fc.lengths(len(keys), 4)
    got = fc.check_table(fc.model_image(64, keys, lens), 64, fc.expected(keys, lens), lost_ok=True)
    assert len(got.keys) == 64 and len(got.missing) == 1 and got.lost == 3


def _dup(img):
    k = fc.payload(img, "keys")
    s = np.flatnonzero(k)[0]
    rs = fc.region_slots(8192)
    free = next(x for x in range(s // rs * rs, s // rs * rs + rs) if k[x] == 0)
    k[free] = k[s]  # same region, counts zero


def _too_far(img):
    k, p, b = (fc.payload(img, x) for x in ("keys", "packets", "bytes"))
    s = np.flatnonzero(k[:4096])[0]
    t = 4096 + np.flatnonzero(k[4096:] == 0)[0]
    k[t], p[t], b[t] = k[s], p[s], b[s]
    k[s] = p[s] = b[s] = 0


def _off_by_one(img):
    fc.payload(img, "packets")[np.flatnonzero(fc.payload(img, "keys"))[3]] += 1


def _bytes_off_by_one(img):
    fc.payload(img, "bytes")[np.flatnonzero(fc.payload(img, "keys"))[5]] -= 1


def _carry(img):
    s = np.flatnonzero(fc.payload(img, "keys"))[7]
    fc.payload(img, "packets")[s] += 1
    b = fc.payload(img, "bytes")
    b[s] = np.uint64((int(b[s]) - (1 << 40)) % (1 << 64))  # the packed word's carry, as it looks after the unpack


def _ghost_count(img):
    fc.payload(img, "bytes")[np.flatnonzero(fc.payload(img, "keys") == 0)[0]] = 60


def _front_guard(img):
    img["packets"][fc.GUARD - 1] = 0


def _rear_guard(img):
    img["keys"][len(img["keys"]) - fc.GUARD] = 0


def _input_guard(img):
    img["lens_in"][3] ^= 0xFF


def _input_payload(img):
    img["lens_in"][fc.GUARD + 3] ^= 0xFF


def _stats3(img):
    a = img["stats"]
    a[len(a) - fc.GUARD:len(a) - fc.GUARD + 8] = 0


def _lost_one(img):
    k, p, b = (fc.payload(img, x) for x in ("keys", "packets", "bytes"))
    s = np.flatnonzero(k)[0]
    k[s] = p[s] = b[s] = 0


def _zero_key(img):
    fc.payload(img, "stats")[0] -= 1


def _lost_unasked(img):
    """One flow's packets moved to stats[2]: conserved, but nothing may be lost with room in the table."""
    k, p, b = (fc.payload(img, x) for x in ("keys", "packets", "bytes"))
    s = np.flatnonzero(k)[0]
    fc.payload(img, "stats")[2] += p[s]
    k[s] = p[s] = b[s] = 0


FAULTS = {"duplicate key": _dup, "wrong region": _too_far, "wrong count": _off_by_one,
          "wrong count (bytes)": _bytes_off_by_one, "carry": _carry, "empty slot count": _ghost_count,
          "guard (front)": _front_guard, "guard (rear)": _rear_guard, "guard (input)": _input_guard,
          "input changed": _input_payload, "stats[3]": _stats3, "conservation": _lost_one, "key 0": _zero_key,
          "lost": _lost_unasked}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_checker_fails_on_each_injected_fault(fault):
    img, exp = fresh()
    keys, lens, _ = standin()
    inputs = {"lens_in": lens}
    img.update({k: v for k, v in fc.blank_image({"lens_in": lens.nbytes}).items()})
    fc.payload(img, "lens_in", np.uint32)[:] = lens
    fc.check_table(img, 8192, exp, calls=2, inputs=inputs)  # correct before the fault
    FAULTS[fault](img)
    with pytest.raises(FlowTableError) as e:
        fc.check_table(img, 8192, exp, calls=2, inputs=inputs)
    assert e.value.kind == fault.split(" (")[0], str(e.value)
    if fault == "wrong region":
        assert "partition constant" in str(e.value)


def test_checker_requires_full_regions_where_keys_are_lost():
    """lost_ok: a lost key is accepted only where its region has no empty slot."""
    keys, lens, exp = standin()
    img = fc.model_image(8192, keys, lens)
    _lost_unasked(img)
    with pytest.raises(FlowTableError) as e:
        fc.check_table(img, 8192, exp, lost_ok=True)
    assert e.value.kind == "lost with room"


def test_filter_restatement_pieces():
    """The six packets parse to the stacks the filter cases assume, a source-port spec matches one direction only, and
    filter_expect's first sequence numbers follow the own-matching packets."""
    _, s, _ = fc.filter_kinds()
    bit = lambda i, p: (int(s["proto_mask"][i]) >> p) & 1  # noqa: E731
    assert bit(fc.UF, oracle.P_UDP) and bit(fc.TR, oracle.P_TCP) and bit(fc.ARP, oracle.P_ARP) and bit(fc.V6, oracle.P_IPV6)
    case = fc.filter_case([fc.UR, fc.UF, fc.UR, fc.TF, fc.ARP, fc.UF], [5, 5, 5, 6, 0, 5])
    spec = oracle.make_spec(src_port=fc.SP)
    assert fc.filter_own(case, spec).tolist() == [False, True, False, True, False, True]
    m, st, tab = fc.filter_expect(case, spec, seq_base=100)
    assert m.tolist() == [0, 1, 1, 1, 0, 1] and tab == {(1 << 32) | 5: 101, (1 << 32) | 6: 103}
    assert (st["matched_udp_flows"], st["matched_tcp_flows"], st["matched_packets"]) == (1, 1, 4)
    assert fc.filter_own(case, oracle.make_spec()).all()


# ------------------------------------------------------------------ GPU: count and merge
def run_count(engine, capacity: int, keys, lens, calls: int = 1, via: str = "keys"):
    """`calls` calls of the count over one guarded arena; returns (image, the input columns as uploaded)."""
    import torch

    keys = np.ascontiguousarray(keys, np.uint32)
    lens = np.ascontiguousarray(lens, np.uint32)
    n = len(keys)
    if via == "summary":
        s = np.zeros(n, abi.SUMMARY_DTYPE)
        s["hash5"] = keys
        ar = fc.Arena(capacity, summary_in=s, lens_in=lens)
        call, col = engine.flow_count_device, ar.out("summary_in")
    else:
        ar = fc.Arena(capacity, keys_in=keys, lens_in=lens)
        call, col = engine.flow_count_keys_device, ar.out("keys_in")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(calls):
        call(col, ar.out("lens_in"), n, ar.out("keys"), ar.out("packets"), ar.out("bytes"), capacity, ar.out("stats"), st)
    torch.cuda.synchronize()
    return ar.host(), ar.inputs


def count_and_check(engine, capacity, keys, lens, calls=1, lost_ok=False, exp=None, via="keys") -> fc.Checked:
    img, inputs = run_count(engine, capacity, keys, lens, calls, via)
    return fc.check_table(img, capacity, exp or fc.expected(keys, lens), calls, lost_ok, inputs)


def assert_same_table_from_summaries(engine, capacity, keys, lens, exp, img, calls=1):
    """pcppx_flow_count_device over a synthetic summary array (only hash5 is read) gives the same table as the dense
    column gave in `img`: the kernel's other instance, held to the same rules."""
    other, inputs = run_count(engine, capacity, keys, lens, calls, via="summary")
    fc.check_table(other, capacity, exp, calls, inputs=inputs)
    assert fc.as_dict(other) == fc.as_dict(img)


@pytest.mark.gpu
@pytest.mark.parametrize("n,column,capacity", fc.n_edge_table(), ids=lambda v: str(v))
def test_gpu_count_n_edges(engine, n, column, capacity):
    """n at the lane (1, 63-65, 1023-1025), batch (6144 +- 1, 2 x 6144 +- 1) and grid (256 x 6144 +- 1, 257 x 6144 + 1)
    edges of flow_count_kernel's fetch / valid mask and of the merge's round loop, with all-distinct keys, one key and
    all-zero keys, one packet of length 0 and one of 65535."""
    keys, lens = fc.n_edge_keys(n, column), fc.lengths(n, n)
    exp = fc.expected(keys, lens)
    img, inputs = run_count(engine, capacity, keys, lens)
    got = fc.check_table(img, capacity, exp, inputs=inputs)
    assert len(got.keys) == {"distinct": n, "one": 1, "zero": 0}[column]
    if (n, column) in fc.SUMMARY_TOO:
        assert_same_table_from_summaries(engine, capacity, keys, lens, exp, img)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", fc.LADDER)
def test_gpu_count_capacity_ladder(engine, capacity):
    """Capacities 1 and 2 (log2r 0 and 1), the region-rule changes 4096 -> 8192 and 2^21 -> 2^22 (flow_partitions_log2),
    half full, two calls into one table (the merge finds its keys again and adds)."""
    keys = fc.ladder_keys(capacity)
    got = count_and_check(engine, capacity, keys, fc.lengths(len(keys), capacity, edges=False), calls=2)
    assert len(got.keys) == fc.ladder_flows(capacity)


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [1, 2, 64, 4096])
@pytest.mark.parametrize("extra", [0, 1])
def test_gpu_count_full_region(engine, capacity, extra):
    """A region at 100 % load (the merge's probe loop runs to its last step, `probe <= rm`), and one distinct key more
    than it holds: exactly one key of the input is missing and stats[2] is that key's packet count."""
    pool = full_region_keys(capacity, extra)
    keys = fc.cycle(pool, 3 * len(pool))
    lens = fc.lengths(len(keys), capacity + extra, edges=False)
    got = count_and_check(engine, capacity, keys, lens, lost_ok=bool(extra))
    assert len(got.keys) == capacity and len(got.missing) == extra
    assert got.lost == 3 * extra


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_gpu_count_full_region_beside_a_sparse_one(engine, extra):
    """Capacity 8192: partition 1 full (or one key over), partition 0 with 10 keys -- a full region spills neither into
    its neighbour nor past the table: region 0 holds its 10 keys and nothing else."""
    p1, p0 = two_region_keys(extra)
    pool = np.concatenate([p1, p0])
    keys = fc.cycle(pool, 2 * len(pool))
    got = count_and_check(engine, 8192, keys, fc.lengths(len(keys), 8, edges=False), lost_ok=bool(extra))
    assert len(got.missing) == extra and got.lost == 2 * extra
    assert np.isin(got.missing, p1).all()
    low = got.keys[got.slots < 4096]
    assert sorted(low.tolist()) == sorted(p0.tolist())
    assert int((got.slots >= 4096).sum()) == 4096


@pytest.mark.gpu
def test_gpu_count_region_wrap(engine):
    """Probe chains that reach a region's last slot come back to the region's first slot ((r + 1) & rm in the merge): 600
    keys of region slot 4095 in the table's last region -- a spill would land in the rear guard -- and 600 of slots
    4094 / 4095 in region 0, whose spill would enter region 1."""
    last, first = wrap_keys()
    pool = np.concatenate([last, first])
    keys = fc.cycle(pool, 3 * len(pool))
    got = count_and_check(engine, 1 << 21, keys, fc.lengths(len(keys), 9))
    assert_wrapped_run(got, 1 << 21, 511, 600)
    assert_wrapped_run(got, 1 << 21, 0, 600)


@pytest.mark.gpu
def test_gpu_count_region_wrap_by_the_overflow_atomics(engine):
    """The same wrap in flow_region_add_atomic, the path of a full partition queue: 8 blocks each queue all 600 keys of
    the last region, 4800 records for a queue of 4216, so the rest are added with atomics on the region and probe
    across its end."""
    last, _ = wrap_keys()
    keys = fc.cycle(last, 8 * BATCH)
    got = count_and_check(engine, 1 << 21, keys, fc.lengths(len(keys), 10))
    assert_wrapped_run(got, 1 << 21, 511, 600)


@pytest.mark.gpu
@pytest.mark.parametrize("batches", [1, 3])
def test_gpu_count_lds_collisions(engine, batches):
    """flow_count_kernel's LDS table: 4000 distinct keys whose home is its last slot, 8191 -- one probe chain that wraps
    to slot 0 ((slot + 1) & (kFlowLds - 1)); in one batch and over three blocks' batches."""
    keys = fc.cycle(count_lds_keys(), batches * BATCH)
    got = count_and_check(engine, 4096, keys, fc.lengths(len(keys), batches))
    assert len(got.keys) == 4000


@pytest.mark.gpu
def test_gpu_merge_lds_collisions_and_mid_queue_flush(engine):
    """flow_merge_kernel's LDS table: 3000 keys whose home is its last slot, 4095 (the wrap), each queued by 4 blocks: the
    merge flushes above 2048 used slots while records of the flushed keys are still to come, and finds them again in
    the region."""
    keys = fc.cycle(merge_lds_keys(), 4 * BATCH)
    lens = fc.lengths(len(keys), 5)
    exp = fc.expected(keys, lens)
    img, inputs = run_count(engine, 4096, keys, lens, calls=2)
    got = fc.check_table(img, 4096, exp, calls=2, inputs=inputs)
    assert len(got.keys) == 3000
    assert_same_table_from_summaries(engine, 4096, keys, lens, exp, img, calls=2)


@pytest.mark.gpu
@pytest.mark.parametrize("column", fc.HOT_COLUMNS)
def test_gpu_count_hot_flows(engine, column):
    """The hot-flow rule of flow_count_kernel's flush (more than kHot = 2 packets, at most 1024 kept, first come first
    kept) with two batches per block: 1536 hot flows per batch (512 over the limit are flushed, 1024 kept and met again),
    a Zipf column, and one flow of exactly 2 and one of exactly 3 packets per batch."""
    keys, lens = fc.hot_keys(column), fc.lengths(fc.HOT_N, 6)
    exp = fc.expected(keys, lens)
    img, inputs = run_count(engine, 1 << 21, keys, lens)
    fc.check_table(img, 1 << 21, exp, inputs=inputs)
    if column == "quads":
        assert_same_table_from_summaries(engine, 1 << 21, keys, lens, exp, img)


@pytest.mark.gpu
@pytest.mark.parametrize("n", fc.SPLIT_NS)
def test_gpu_count_launch_split_one_flow(engine, n):
    """launch_flow_count_part's split at kPackedMax = 2^24 - 1: one flow, every length 65535. At n = 2^24 - 1 the flow's
    bytes are the 40-bit field's bound, 2^40 - 2^24 - 2^16 + 1 -- a carry into the packet count would show as `carry`;
    one and 6146 packets more go to a second launch (the `+ done` pointers, the queues reused)."""
    keys = np.full(n, fc.SPLIT_KEY, np.uint32)
    lens = np.full(n, fc.MAX_CAPLEN, np.uint32)
    exp = fc.one_flow(fc.SPLIT_KEY, n, fc.MAX_CAPLEN)
    if n == fc.LAUNCH_MAX:
        assert int(exp.bytes[0]) == fc.BYTES_BOUND
    got = count_and_check(engine, 1 << 21, keys, lens, exp=exp)
    assert len(got.keys) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", fc.SPLIT_NS)
def test_gpu_count_launch_split_many_flows(engine, n):
    """The same split with key i % 100003 + 1 and length 60 + i % 1455: every flow has packets on both sides of the
    cut."""
    keys, lens = fc.split_column2(n)
    got = count_and_check(engine, 1 << 21, keys, lens)
    assert len(got.keys) == 100003


@pytest.mark.gpu
def test_gpu_oversize_and_bad_descriptors_count_under_key_zero(engine):
    """Why the 40-bit byte field is enough: a parse gives key 0 to every packet with caplen > PCPPX_MAX_CAPLEN (OVERSIZE)
    or a descriptor past data_len (BAD_DESC) -- here caplens 65536, 70000 and 0xFFFFFFFF among plain packets -- and the
    count sums key-0 bytes in 64 bits into stats[1]."""
    import torch

    from pcapplusplus_amd.engine import to_device

    b, s, big, opts = oversize_batch()
    caps = b.caplens
    data, d_offs, d_caps = to_device(b)
    ar = fc.Arena(4096, sizes={**fc.table_sizes(4096), "flow_keys": 4 * b.n, "summary": 32 * b.n})
    st = torch.cuda.current_stream().cuda_stream
    engine.parse_device(data, d_offs, d_caps, b.n, b.linktype, opts, ar.out("summary"), None, st,
                        flow_keys=ar.out("flow_keys"))
    engine.flow_count_keys_device(ar.out("flow_keys"), d_caps, b.n, ar.out("keys"), ar.out("packets"), ar.out("bytes"),
                                  4096, ar.out("stats"), st)
    torch.cuda.synchronize()
    img = ar.host()
    col = fc.payload(img, "flow_keys", np.uint32)
    assert np.array_equal(col, s["hash5"]) and (col[big] == 0).all()
    exp = fc.expected(s["hash5"], caps)
    assert exp.zero_bytes > 1 << 32  # past one word: 64-bit sums
    fc.check_table({k: img[k] for k in ("keys", "packets", "bytes", "stats")}, 4096, exp)
    fc.check_guards(img)


STREAM_NS = (10, 3_000_000, 10, 1 << 20)


def _stream_sequence(eng, ns):
    """Calls of changing n, alternating between two tables (capacity 2^21 and 4096: 512 partitions and 1) and two
    streams, with no synchronisation but the library's own; one synchronise at the end; both tables exact."""
    import torch

    pool = fc.distinct(2000, salt=17)
    caps = (1 << 21, 4096)
    cols = []
    for j, n in enumerate(ns):
        rng = np.random.default_rng(100 + n + j)
        cols.append((pool[rng.integers(0, len(pool), n)], fc.lengths(n, 200 + j)))
    arenas = [fc.Arena(cap, **{f"k{j}": cols[j][0] for j in range(len(ns)) if j % 2 == t},
                       **{f"l{j}": cols[j][1] for j in range(len(ns)) if j % 2 == t}) for t, cap in enumerate(caps)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()  # the uploads; from here on the library orders its own work
    for j, n in enumerate(ns):
        ar = arenas[j % 2]
        eng.flow_count_keys_device(ar.out(f"k{j}"), ar.out(f"l{j}"), n, ar.out("keys"), ar.out("packets"),
                                   ar.out("bytes"), caps[j % 2], ar.out("stats"), streams[(j // 2 + j) % 2].cuda_stream)
    torch.cuda.synchronize()
    for t, cap in enumerate(caps):
        mine = [c for j, c in enumerate(cols) if j % 2 == t]
        exp = fc.expected(np.concatenate([k for k, _ in mine]), np.concatenate([ln for _, ln in mine]))
        fc.check_table(arenas[t].host(), cap, exp, inputs=arenas[t].inputs)


@pytest.mark.gpu
def test_gpu_count_scratch_streams_and_changing_shapes(engine):
    """The context's flow scratch (Scratch::acquire in pcppx_capi.cpp's flow_count): the queues regrow in stream order
    when n grows (10 -> 3M), shrink back in use (-> 10 -> 2^20), the partition count changes with the table (512 / 1,
    the merge resets only its own fill counters), and a call on one stream waits for the previous call's work on the
    other by the library's own event. Then the same on a fresh Engine with n in reverse order."""
    from pcapplusplus_amd.engine import Engine

    _stream_sequence(engine, STREAM_NS)
    eng = Engine(0)
    try:
        _stream_sequence(eng, STREAM_NS[::-1])
    finally:
        eng.close()


# ------------------------------------------------------------------ GPU: the filter's table
def flows_case(hashes, pattern) -> fc.FilterCase:
    """Flow f's packets are `pattern`'s kinds (UDP for even f, the TCP twin for odd f), interleaved flow by flow."""
    kinds, h5 = [], []
    for kind in pattern:
        for f, h in enumerate(hashes):
            kinds.append(kind + 2 if f % 2 and kind in (fc.UF, fc.UR) else kind)
            h5.append(int(h))
    return fc.filter_case(kinds, h5)


def assert_filter(img, case, spec, capacity, seq_base=0):
    want_m, want_st, want_tab = fc.filter_expect(case, spec, seq_base)
    tab = fc.filter_table(img, capacity)
    got_m = fc.payload(img, "matched", np.uint8)
    assert np.array_equal(got_m, want_m), np.flatnonzero(got_m != want_m)[:10]
    assert fc.filter_stats(img) == want_st
    assert tab == want_tab
    return tab


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [1, 2, 8, 64])
@pytest.mark.parametrize("spec_kind", ["any", "src_port"])
def test_gpu_filter_table_exactly_full(engine, capacity, spec_kind):
    """filter_mark_kernel's probe loop at 100 % load: exactly `capacity` matched flows, UDP and TCP, both directions, an
    ARP and an IPv6 packet that match nothing under the port spec: flow_table_full == 0, verdicts, every counter and
    the table {key: first} equal the restatement's."""
    spec = oracle.make_spec() if spec_kind == "any" else oracle.make_spec(src_port=fc.SP)
    case = flows_case(fc.distinct(capacity, salt=31), (fc.UR, fc.UF, fc.UR, fc.UF))
    if spec_kind == "src_port":  # two packets that match nothing and are no flow of the table
        case = fc.filter_case(np.concatenate([case.kinds, [fc.ARP, fc.V6]]), np.concatenate([case.hash5, [0, 77]]))
    tab = assert_filter(fc.run_filter(engine, case, spec, capacity), case, spec, capacity)
    assert len(tab) == capacity


@pytest.mark.gpu
@pytest.mark.parametrize("capacity", [1, 2, 8, 64])
def test_gpu_filter_table_one_flow_too_many(engine, capacity):
    """capacity + 1 matched flows: which flow finds no slot is the hardware's choice; it is the only difference. Its
    packets match only on their own, it is no counted flow, flow_table_full counts its own-matching packets; every
    stored flow's verdicts and `first` are the restatement's."""
    spec = oracle.make_spec(src_port=fc.SP)
    hashes = fc.distinct(capacity + 1, salt=33)
    case = flows_case(hashes, (fc.UR, fc.UF, fc.UR, fc.UF))
    img = fc.run_filter(engine, case, spec, capacity)
    want_m, want_st, want_tab = fc.filter_expect(case, spec)
    tab = fc.filter_table(img, capacity)
    assert len(tab) == capacity and len(want_tab) == capacity + 1
    (left,) = set(want_tab) - set(tab)
    assert tab == {k: v for k, v in want_tab.items() if k != left}
    own = fc.filter_own(case, spec)
    of_left = case.hash5 == (left & 0xFFFFFFFF)
    want_m = np.where(of_left, own, want_m).astype(np.uint8)
    assert np.array_equal(fc.payload(img, "matched", np.uint8), want_m)
    f = int(np.flatnonzero(hashes == (left & 0xFFFFFFFF))[0])
    want_st["matched_tcp_flows" if f % 2 else "matched_udp_flows"] -= 1
    want_st["matched_packets"] = int(want_m.sum())
    want_st["flow_table_full"] = int((own & of_left).sum())
    assert want_st["flow_table_full"] == 2
    assert fc.filter_stats(img) == want_st


@pytest.mark.gpu
@pytest.mark.parametrize("capacity,count,slot", [(64, 40, 63), (8, 8, 7)])
def test_gpu_filter_table_wrap_and_collisions(engine, capacity, count, slot):
    """Colliding keys whose slot is the table's last: the chains of filter_mark_kernel and filter_apply_kernel wrap at
    slot capacity - 1 to slot 0 ((slot + 1) & m) and stay in the table (a spill would land in the rear guards)."""
    spec = oracle.make_spec(src_port=fc.SP)
    case = flows_case(fc.filter_slot_keys(count, capacity, slot), (fc.UR, fc.UF, fc.UR))
    img = fc.run_filter(engine, case, spec, capacity)
    assert_filter(img, case, spec, capacity)
    used = np.flatnonzero(fc.payload(img, "flow_keys", np.uint64))
    assert sorted(used.tolist()) == sorted(((slot + j) % capacity) for j in range(count))


@pytest.mark.gpu
def test_gpu_filter_key_zero_is_one_flow(engine):
    """Packets without a 5-tuple (ARP, hash5 0) under the match-everything spec: one flow with key 1 << 32 | 0 -- a used
    slot, not an empty one; counted in matched_packets, in neither matched_tcp_flows nor matched_udp_flows."""
    spec = oracle.make_spec()
    case = fc.filter_case([fc.ARP, fc.UF, fc.ARP, fc.TF, fc.ARP, fc.V6], [0, 5, 0, 6, 0, 7])
    img = fc.run_filter(engine, case, spec, 8)
    tab = assert_filter(img, case, spec, 8)
    st = fc.filter_stats(img)
    assert tab[1 << 32] == 0 and len(tab) == 4
    assert (st["matched_packets"], st["matched_udp_flows"], st["matched_tcp_flows"], st["arp_count"]) == (6, 2, 1, 3)


def order_case(n: int, own_at, other_at, h: int = 0xF10F):
    """n packets that match nothing on their own, each a flow of its own, except flow h: reverse packets at `other_at`,
    own-matching forward packets at `own_at`."""
    kinds = np.full(n, fc.UR)
    h5 = fc.distinct(n, salt=41)
    assert h not in h5
    kinds[list(own_at)] = fc.UF
    h5[list(own_at) + list(other_at)] = h
    return fc.filter_case(kinds, h5)


TRIPLES = ((3, 10, 40), (63, 64, 65), (255, 256, 257))


@pytest.mark.gpu
@pytest.mark.parametrize("a,b,c", TRIPLES, ids=lambda v: str(v))
@pytest.mark.parametrize("cut", ["none", "after_a", "after_b"])
def test_gpu_filter_order_rule_at_wave_block_and_call_edges(engine, a, b, c, cut):
    """"Matched if an earlier packet of the flow matched": a flow's packets at a < b < c, only b matching on its own,
    inside one wave, across the wave edge 63 | 64 | 65 and the block edge 255 | 256 | 257, in one call and cut into two
    calls after a and after b (seq_base continues): a unmatched, b and c matched, the flow counted once."""
    spec = oracle.make_spec(src_port=fc.SP)
    case = order_case(c + 7, (b,), (a, c))
    cuts = {"none": (), "after_a": (b,), "after_b": (c,)}[cut]
    img = fc.run_filter(engine, case, spec, 64, cuts=cuts, seq_base=1000)
    tab = assert_filter(img, case, spec, 64, seq_base=1000)
    m = fc.payload(img, "matched", np.uint8)
    assert (int(m[a]), int(m[b]), int(m[c]), int(m.sum())) == (0, 1, 1, 2)
    assert tab == {(1 << 32) | 0xF10F: 1000 + b} and fc.filter_stats(img)["matched_udp_flows"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("p,q", [(5, 9), (100, 300)])
def test_gpu_filter_two_own_matches_count_one_flow(engine, p, q):
    """Two own-matching packets of one flow in one wave and in two blocks: the flow is counted once (own && first == seq
    holds for the earlier one only) and `first` is the smaller sequence number (atomicMax over ~seq)."""
    spec = oracle.make_spec(src_port=fc.SP)
    case = order_case(q + 3, (p, q), (q + 1,))
    img = fc.run_filter(engine, case, spec, 8, seq_base=7)
    tab = assert_filter(img, case, spec, 8, seq_base=7)
    assert tab == {(1 << 32) | 0xF10F: 7 + p}
    st = fc.filter_stats(img)
    assert (st["matched_udp_flows"], st["matched_packets"]) == (1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("seq_base", [0, (1 << 32) - 3, (1 << 63) - 3])
def test_gpu_filter_seq_base(engine, seq_base):
    """Sequence numbers across 2^32 (a batch of 8 from 2^32 - 3) and near 2^63, two consecutive calls continuing the
    numbering: verdicts and counters are the seq_base-0 run's, `first` is shifted by seq_base."""
    spec = oracle.make_spec(src_port=fc.SP)
    kinds = [fc.UR, fc.UF, fc.UR, fc.TR, fc.TR, fc.TF, fc.ARP, fc.UR,  # flow 5 matches at 1, flow 6 at 5, across the
             fc.UF, fc.TR, fc.UR, fc.UF, fc.V6, fc.TF, fc.UR, fc.TR]   # second call flow 8 at 11, flow 9 never
    h5 = [5, 5, 5, 6, 6, 6, 0, 8, 5, 6, 8, 8, 7, 6, 9, 9]
    case = fc.filter_case(kinds, h5)
    img = fc.run_filter(engine, case, spec, 8, cuts=(8,), seq_base=seq_base)
    tab = assert_filter(img, case, spec, 8, seq_base=seq_base)
    zero = fc.run_filter(engine, case, spec, 8, cuts=(8,), seq_base=0)
    assert np.array_equal(fc.payload(img, "matched", np.uint8), fc.payload(zero, "matched", np.uint8))
    assert fc.filter_stats(img) == fc.filter_stats(zero)
    assert tab == {k: v + seq_base for k, v in fc.filter_table(zero, 8).items()}
    assert tab == {(1 << 32) | 5: seq_base + 1, (1 << 32) | 6: seq_base + 5, (1 << 32) | 8: seq_base + 11}
