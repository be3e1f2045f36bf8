"""The open-addressed tables of pcppx_defrag_device, pcppx_defrag6_device and pcppx_tcpstream_device on keys aimed at
their probe loops (tests/table_cases.py): chains of every key of a batch on one home slot, chains that wrap past the
last slot, key 0 displaced, both sides of each doubling of the table, a table at its densest, lanes of one wave racing
for one slot, lookups that walk a displaced chain to a key or to a free slot.

CPU: the model's constants are the kernels'; each case reaches what it is named for (a failure there is the
generator's, not the kernel's); pcppx_*_reference equals the brute-force restatement of the contract on every case,
whole buffers; a numpy stand-in of slot_of() passes on the cases' key columns and fails on them with each of three
faults. GPU: the device equals the reference on every case, index-only and with data, twice on the default stream and
once on a second one, and a call on a small table is unaffected by a call on a large one before it.
"""
from __future__ import annotations

import re
from dataclasses import replace

import numpy as np
import pytest

import defrag6_cases as d6
import defrag_cases as dc
import table_cases as tb
import tcpstream_cases as tc
from pcapplusplus_amd import abi

CSRC = abi.PKG_DIR / "csrc"
GROUP = tb.group_table_cases()
GROUP_BY_NAME = {c.name: c for c in GROUP}
# defrag6: the same cases with families = V4, and cases with IPv6 groups in the same chains with V4 | V6
GROUP6 = [replace(d6.widen(c, d6.V4), name=c.name + "_v4") for c in GROUP] + \
    [replace(d6.widen(c, d6.V4 | d6.V6), name=c.name + "_v4v6") for c in tb.group_table_cases(v6_every=2)]
GROUP6_BY_NAME = {c.name: c for c in GROUP6}
STREAM = tb.stream_table_cases()
STREAM_BY_NAME = {c.name: c for c in STREAM}
SMALL = 3200  # the stream() model's bound in tests/test_defrag.py
STANDIN_BUDGET = 600_000  # probes of all lanes: what the lockstep stand-in walks in a second (all but dense_one_home)


def name_of(c):
    return c.name


# ---------------------------------------------------------------- CPU: the model
def test_model_constants_are_the_kernels():
    """Both multipliers from the .hip sources, the table's minimum and the per-candidate block from pcppx_internal.h,
    the size and room rules restated; the block sizes the cases place their members by."""
    for name in ("pcppx_defrag.hip", "pcppx_tcpstream.hip"):
        txt = (CSRC / name).read_text()
        (mult,) = set(re.findall(r"\*\s*(0x[0-9A-Fa-f]+)u\)\s*>>\s*t\.shift", txt))
        assert int(mult, 16) == tb.MULT
        assert re.search(r"s = \(s \+ 1\) & \(t\.slots - 1\);", txt)
    seg = re.search(r"return sid \* (0x[0-9A-Fa-f]+)u \+ rel;", (CSRC / "pcppx_tcpstream.hip").read_text())
    assert int(seg.group(1), 16) == tb.SEG_MULT
    txt = (CSRC / "pcppx_internal.h").read_text()
    for const, want in (("kDefragMinSlots", tb.MIN_SLOTS), ("kTcpsMinSlots", tb.MIN_SLOTS),
                        ("kDefragCandPerBlock", tb.CAND_PER_BLOCK), ("kTcpsCandPerBlock", tb.CAND_PER_BLOCK),
                        ("kDefragBlockPk", dc.BLOCK), ("kTcpsBlockPk", tc.BLOCK)):
        assert int(re.search(rf"{const}\s*=\s*(\d+)", txt).group(1)) == want, const
    assert (tb.MULT * tb.MINV) & tb.M32 == 1
    rooms = (0, 1, 32, 33, 64, 65, 1024, 1025, 4096)
    assert [tb.slots_for(r) for r in rooms] == [64, 64, 64, 128, 128, 256, 2048, 4096, 8192]
    assert tb.slots_for(1 << 31) == 1 << 31 and tb.slots_for((1 << 30) + 1) == 1 << 31
    assert [tb.room_for(10, m) for m in (0, 9, 10, 11)] == [10, 9, 10, 10]


def test_keys_at_and_layout():
    for slots in (64, 128, 8192):
        for h in (0, 1, slots // 2, slots - 1):
            keys = tb.keys_at(h, slots, 40)
            assert len(set(keys)) == 40 and {tb.home(k, slots) for k in keys} == {h}
            assert all(0 <= k <= tb.M32 for k in keys)
    assert tb.keys_at(0, 128, 3)[0] == 0
    lay = tb.layout(tb.keys_at(126, 128, 5), 128)
    assert (sorted(lay.occupied), lay.displacement, lay.wrapped) == ([0, 1, 2, 126, 127], 4, True)
    keys = tb.keys_at(10, 64, 3) + tb.keys_at(11, 64, 2)
    for order in (keys, keys[::-1], keys[2:] + keys[:2]):  # the occupied set does not depend on the order
        assert sorted(tb.layout(order, 64).occupied) == [10, 11, 12, 13, 14]
    assert tb.seg_home(18, 0, 64) == tb.home((18 * tb.SEG_MULT) & tb.M32, 64)


# ---------------------------------------------------------------- CPU: the cases reach what they are named for
def _chain_checks(c, lanes, table="group"):
    m = c.meta
    keys, slots, kind = m["keys"], m["slots"], m["kind"]
    lay = tb.layout(lanes, slots)
    assert set(lanes) >= set(keys) and len(lay.where) == len(set(lanes))
    homes = [tb.home(k, slots) for k in keys]
    if kind in ("one_home", "wrap", "step", "race", "overflow", "dense_one_home"):
        assert len(set(homes)) == 1 and tb.layout(keys, slots).displacement == len(keys) - 1
    if kind in ("wrap", "step", "race", "overflow", "dense_one_home", "dense_run", "key0", "lookup_absent"):
        assert lay.wrapped
    if kind == "one_home":
        assert not lay.wrapped and len(keys) == 32
    if c.name.startswith("home_last_slot"):
        assert homes[0] == slots - 1
    if kind == "key0":  # key 0, whose members come behind the chain's, rests behind the chain
        assert keys[-1] == 0 and tb.home(0, slots) == 0 and lay.where[0] >= 1 and 0 in lay.occupied
        assert lay.where[0] == len(keys) - 1 - 6 and max(i for i, k in enumerate(lanes) if k) < lanes.index(0)
    if kind == "step":
        room = m["candidates"]
        assert room in tb.STEP_EDGES and c.n == room and slots == tb.slots_for(room) and homes[0] == slots - 3
    if kind.startswith("dense"):
        assert c.n == m["candidates"] == tb.DENSE_N and slots == 8192
        if table == "group":
            assert len(keys) * 4 == slots  # a load of exactly 25 %
        else:  # 1,024 connections in the connection table; 4,096 data segments in the segment table
            assert len(keys) * 8 == slots and m["candidates"] * 2 == slots
    if kind == "dense_run":  # a solid run of slots, nothing displaced but the last key, which walks all of it
        first = tb.home(keys[0], slots)
        assert lay.occupied == frozenset((first + j) & (slots - 1) for j in range(len(keys)))
        d = {k: (s - tb.home(k, slots)) & (slots - 1) for k, s in lay.where.items()}
        assert d[keys[-1]] == len(keys) - 1 and sum(d.values()) == len(keys) - 1
    if kind == "race":
        assert len(keys) == 8


def test_group_cases_reach_what_they_name():
    assert [c.name for c in GROUP] == [c.name[:-5] for c in GROUP6[len(GROUP):]]
    for c in GROUP + GROUP6:
        lanes = tb.group_lanes(c)
        _chain_checks(c, lanes)
        kind = c.meta["kind"]
        mod = d6 if isinstance(c, d6.Case) else dc
        t = abi.defrag_totals_dict(mod.brute(c).totals)
        assert t["candidates"] == c.meta["candidates"] or kind == "lookup_absent"
        if kind == "race":
            rows = np.nonzero(c.info["ip_status"] & 15 == abi.IPR_FRAGMENT)[0]
            if c.n == 64:  # each wave step sees the eight keys eight times
                assert all(sorted(lanes[j:j + 8]) == sorted(c.meta["keys"]) for j in range(0, 64, 8))
            else:
                for k in c.meta["keys"]:
                    assert len({int(i) // dc.BLOCK for i in rows if int(c.info["ip_key"][i]) == k}) == 8
        if kind == "unclean":
            assert (t["reassembled"], t["left_frags"], t["merged_frags"]) == (20, 67, 40)
        elif kind == "overflow":
            assert (t["overflow"], t["candidates"], c.max_fragments) == (1, 64, 63)
        elif kind == "lookup_absent":
            keys, slots = c.meta["keys"], c.meta["slots"]
            chain = tb.layout(keys[:-1], slots)
            assert tb.home(keys[-1], slots) in chain.occupied and chain.wrapped
            assert (t["reassembled"], t["left_frags"], t["candidates"]) == (30, 2, 61)
            assert int(c.info["ip_key"][66]) in keys[:-1] and int(c.summary["n_layers"][66]) >= 1
        else:  # every candidate is merged: nothing passes by being LEFT
            assert t["left_frags"] == 0 and t["merged_frags"] == t["candidates"]
            assert t["reassembled"] == len(c.meta["keys"])
    fams = [{bool(s & abi.IPR_F_IPV6) for s in c.info["ip_status"][c.info["ip_status"] & 15 == abi.IPR_FRAGMENT]}
            for c in GROUP6[len(GROUP):]]
    assert all(f == {False, True} for f in fams)  # both families in the same chains


def test_stream_cases_reach_what_they_name():
    for c in STREAM:
        m = c.meta
        lanes = tb.stream_lanes(c)
        assert len(lanes) == m["candidates"]
        got = tc.brute(c)
        t = abi.tcpstream_totals_dict(got.totals)
        assert t["candidates"] == m["candidates"] and t["overflow"] == 0
        if not m["kind"].startswith("seg"):
            _chain_checks(c, lanes, "stream")
            assert t["left"] == 0 and t["streams"] == 2 * len(m["keys"])
            if m["kind"] == "race" and c.n == 64:
                assert all(sorted(lanes[j:j + 8]) == sorted(m["keys"]) for j in range(0, 64, 8))
            continue
        # the segment table: sid = 2 * slot + side is the builder's because every connection rests on its home slot
        slots, target, words = m["slots"], m["seg_target"], m["seg_words"]
        assert tb.layout(m["keys"], slots).displacement == 0 and slots == tb.slots_for(m["candidates"])
        at_home = [w for w in words if tb.seg_home(*w, slots) == target]
        assert len(at_home) >= (64 if m["kind"] == "seg_many" else 24) and len(set(words)) == len(words)
        lay = tb.layout(words, slots, lambda w: tb.seg_home(*w, slots))
        assert lay.displacement >= len(at_home) - 1
        if m["kind"] != "seg":
            assert target == slots - 3 and lay.wrapped
        if "seg_end" in m:  # the last end is not in the table and is looked for along the whole chain
            assert tb.seg_home(*m["seg_end"], slots) == target and m["seg_end"] not in words
        recs = got.records()
        if m["kind"] == "seg_left":
            assert (t["streams"], int(recs[0]["side"])) == (1, 1) and t["left"] == m["candidates"] - 1
            continue
        assert t["left"] == 0 and t["streams"] == (8 if m["kind"] == "seg_many" else 2)
        data = got.disposition[:c.n] == abi.TCPS_STREAM
        side0 = [j for j, r in enumerate(recs) if int(r["side"]) == 0]
        rels = sorted(int(p) for p, s, d in zip(got.seg_pos[:c.n], got.seg_stream[:c.n], data) if d and int(s) in side0)
        assert rels == sorted(r for _, r in words)  # the words the builder aimed are the contract's (side, rel)
        ooo = [bool(int(r["flags"]) & abi.TCPS_F_OOO) for r in recs if int(r["side"]) == 0]
        assert ooo == [c.name == "seg_ooo"] * len(ooo)


# ---------------------------------------------------------------- CPU: the contract
@pytest.mark.parametrize("case", GROUP, ids=name_of)
def test_defrag_reference_equals_brute_force(case):
    got = dc.run_reference(case)
    dc.assert_same(got, dc.brute(case), case.name)
    if case.meta["kind"] == "overflow":
        dc.assert_untouched(got, case.name)


@pytest.mark.parametrize("case", GROUP6, ids=name_of)
def test_defrag6_reference_equals_brute_force(case):
    got = d6.run_reference(case)
    d6.assert_same(got, d6.brute(case), case.name)
    if case.meta["kind"] == "overflow":
        d6.assert_untouched(got, case.name)


@pytest.mark.parametrize("case", STREAM, ids=name_of)
def test_tcpstream_reference_equals_brute_force(case):
    tc.assert_same(tc.run_reference(case), tc.brute(case), case.name)


@pytest.mark.parametrize("case", [c for c in GROUP if c.n <= SMALL and c.meta["kind"] != "overflow"], ids=name_of)
def test_reassembled_packets_are_what_the_stream_returns(case):
    """As tests/test_defrag.py has it, in source order and in one seeded permutation."""
    for perm in (np.arange(case.n), np.random.default_rng(100).permutation(case.n)):
        c = dc.permuted(case, perm)
        got = dc.run_reference(c)
        st = dc.stream(c)
        packets = dc.reassembled(got)
        assert len(packets) == int(got.totals[abi.DEFRAG_REASSEMBLED]) > 0
        for i, f, pkt in packets:
            assert i in st and st[i] == (pkt, f), (case.name, i)


# ---------------------------------------------------------------- CPU: slot_of() as a numpy stand-in
def _standin_inputs():
    out = []
    for c, lanes in [(c, tb.group_lanes(c)) for c in GROUP] + [(c, tb.stream_lanes(c)) for c in STREAM]:
        slots = c.meta["slots"]
        lay = tb.layout(lanes, slots)
        if sum(((lay.where[k] - tb.home(k, slots)) & (slots - 1)) + 1 for k in lanes) <= STANDIN_BUDGET:
            out.append((c, lanes))
    return out


STANDIN = _standin_inputs()


def test_standin_passes_on_the_cases():
    names = {c.name for c, _ in STANDIN}
    assert {"one_home", "wrap", "home_last_slot", "key0_displaced", "race_tile", "race_blocks", "lookup_absent",
            "dense_run", "step_1024", "step_1025", "seg_many_sides"} <= names
    assert len(STANDIN) == len(GROUP) + len(STREAM) - 2
    for c, lanes in STANDIN:
        tb.check_standin(lanes, c.meta["slots"], tb.absent_keys(c))


@pytest.mark.parametrize("fault, caught_by", [("no_mask", "wrap"), ("lost_cas_claims", "race_tile"),
                                              ("stop_at_mismatch", "one_home")])
def test_each_fault_of_the_standin_is_caught(fault, caught_by):
    """slot_of() without the & (slots - 1), with a lost compare-and-swap taken for a claim, with a lookup that ends at
    the first other key: the named case's check fails for the group table's and the connection table's key column."""
    failed = []
    for c, lanes in STANDIN:
        try:
            tb.check_standin(lanes, c.meta["slots"], tb.absent_keys(c), fault)
        except AssertionError:
            failed.append(c.name)
    assert failed.count(caught_by) == 2, (fault, failed)


# ---------------------------------------------------------------- GPU
def _three_runs(engine, mod, case, untouched: bool = False):
    """Index-only and with data: two calls on the default stream and one on a second stream, all of them the
    reference's buffers (which slot a key gets is the atomics' business; nothing that is put out is)."""
    import torch

    for c in (replace(case, index_only=True), case):
        want = mod.run_reference(c)
        runs = [mod.DeviceRun(c) for _ in range(3)]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        cur = torch.cuda.current_stream().cuda_stream
        runs[0].launch(engine, cur)
        runs[1].launch(engine, cur)
        torch.cuda.synchronize()
        runs[2].launch(engine, side.cuda_stream)
        for k, r in enumerate(runs):
            got = r.result()
            mod.assert_same(got, want, f"{case.name} index_only={c.index_only} run {k}")
            if untouched:
                mod.assert_untouched(got, case.name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GROUP, ids=name_of)
def test_gpu_defrag_tables(engine, case):
    _three_runs(engine, dc, case, case.meta["kind"] == "overflow")


@pytest.mark.gpu
@pytest.mark.parametrize("case", GROUP6, ids=name_of)
def test_gpu_defrag6_tables(engine, case):
    _three_runs(engine, d6, case, case.meta["kind"] == "overflow")


@pytest.mark.gpu
@pytest.mark.parametrize("case", STREAM, ids=name_of)
def test_gpu_tcpstream_tables(engine, case):
    _three_runs(engine, tc, case)


BACK_TO_BACK = [("dense_one_home", "unclean_in_chain"), ("dense_run", "key0_displaced"), ("step_1025", "wrap")]


def _back_to_back(engine, mod, big, small):
    """The larger table first: the context's scratch still holds its groups' positions, totals and candidate records,
    which are not cleared between calls; nothing of them may show in the second call."""
    assert big.meta["slots"] > small.meta["slots"] and big.meta["candidates"] > small.meta["candidates"]
    mod.assert_same(mod.run_device(engine, big), mod.run_reference(big), big.name)
    mod.assert_same(mod.run_device(engine, small), mod.run_reference(small), f"{small.name} after {big.name}")


@pytest.mark.gpu
@pytest.mark.parametrize("big, small", BACK_TO_BACK)
def test_gpu_small_table_after_a_large_one(engine, big, small):
    _back_to_back(engine, dc, GROUP_BY_NAME[big], GROUP_BY_NAME[small])
    _back_to_back(engine, d6, GROUP6_BY_NAME[big + "_v4v6"], GROUP6_BY_NAME[small + "_v4v6"])
    if small in STREAM_BY_NAME:
        _back_to_back(engine, tc, STREAM_BY_NAME[big], STREAM_BY_NAME[small])
    else:
        _back_to_back(engine, tc, STREAM_BY_NAME[big], STREAM_BY_NAME["seg_wrap"])
