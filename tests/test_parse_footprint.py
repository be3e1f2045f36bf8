"""The parse's write footprint, pinned with poisoned, guarded output buffers (footprint_cases.py).

Every other parse test hands the library zero-filled arrays of exactly n records and reads back [:n]: a store past the
records, a store that never happens where the right value is zero, and a consumer that looks at a layer entry past
n_layers all pass there. Here every output sits between two 4096-B guards in an allocation filled with 0x5A, then
0xA5, and is classified byte by byte against a footprint computed from the restatement's records: what must be written
(and holds the restatement's value), what is unspecified (exactly 8 * sum(max_layers - min(n_layers, max_layers))
bytes of a FIXED or PACKED layer array), and what must be untouched (everything else, both guards included).

CPU tests: the footprint computation against hand-written cases, the classifier against injected faults (a numpy
stand-in for the kernel), the pairwise table's coverage, and every CPU pcppx_*_reference consumer run over records whose
unspecified FIXED entries are 0xFF. GPU tests: the table through pcppx_parse_batch_device on two engines (n ascending
on one, descending on the other: context scratch sized by a larger launch must not leak into a smaller one), the fused
parse + reassembly call, the host path (FIXED and DENSE, pageable and page-locked), reused buffers, and the device
consumers over poisoned records.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

import defrag6_cases
import defrag_cases
import dns_cases
import footprint_cases as fc
import frag6_cases
import frag_cases
import http_cases
import oracle
import select_cases
import steer_cases
import tcpstream_cases
import tlsfp_cases
from footprint_cases import FILLS, GUARD, FootprintError, Region
from pcapplusplus_amd import abi

F, P = fc.F, fc.P
LAYER = abi.LAYER_DTYPE.itemsize


# ------------------------------------------------------------------ CPU: the expected footprint, by hand
def _hand_layers(n: int, ml: int) -> np.ndarray:
    """Layer (i, k) holds proto = (10 * i + k) % 250 + 1 and offset = 1000 + 16 * i + k: every entry distinct, no zero."""
    lay = np.zeros((n, ml), abi.LAYER_DTYPE)
    for i in range(n):
        for k in range(ml):
            lay[i, k] = ((10 * i + k) % 250 + 1, 2, 1000 + 16 * i + k, 4, 40)
    return lay


def _entry_set(mask: np.ndarray) -> set:
    e = mask.reshape(-1, LAYER)
    assert bool((e.all(axis=1) | ~e.any(axis=1)).all())  # whole entries
    return set(np.nonzero(e[:, 0])[0].tolist())


def test_expected_footprint_by_hand():
    # 3 packets, max_layers 2, chains of 1, 3 (capped at 2) and 0 layers: cnt = 1, 2, 0
    nl = np.array([1, 3, 0], np.uint8)
    lay = _hand_layers(3, 2)
    fx = fc.fixed_region(nl, 2, lay)
    # FIXED: packet i's row is entries 2i, 2i + 1: written 0 | 2, 3; unspecified 1 | 4, 5
    assert fx.size == 48
    assert _entry_set(fx.must) == {0, 2, 3} and _entry_set(fx.free) == {1, 4, 5}
    e = fx.expect.view(abi.LAYER_DTYPE)
    assert [int(e["proto"][k]) for k in (0, 2, 3)] == [1, 11, 12]  # (0,0) | (1,0), (1,1)
    assert int(fx.free.sum()) == fc.unspecified_bytes(nl, 2) == 8 * (1 + 0 + 2)
    # PACKED: one tile, the chains back to back from entry 0: (0,0), (1,0), (1,1); unspecified 3, 4, 5
    pk = fc.packed_region(nl, 2, lay)
    assert pk.size == 48
    assert _entry_set(pk.must) == {0, 1, 2} and _entry_set(pk.free) == {3, 4, 5}
    e = pk.expect.view(abi.LAYER_DTYPE)
    assert [int(e["proto"][k]) for k in (0, 1, 2)] == [1, 11, 12]
    assert [int(e["offset"][k]) for k in (0, 1, 2)] == [1000, 1016, 1017]
    assert int(pk.free.sum()) == fc.unspecified_bytes(nl, 2) == 24
    # DENSE (host path): the same three entries, and nothing unspecified: bytes 24.. are untouched
    dn, total = fc.dense_region(nl, 2, lay)
    assert total == 3 and _entry_set(dn.must) == {0, 1, 2} and not dn.free.any()
    assert bytes(dn.expect[:24]) == bytes(pk.expect[:24])


def test_expected_packed_footprint_across_tiles():
    # 66 packets, max_layers 2: tile 0 = packets 0-63 (region: entries 0-127), tile 1 = packets 64, 65 (entries 128-131,
    # the region ends at n * max_layers = 132). Chains: packet 0 two layers, packet 63 one, packet 64 none, packet 65 two
    nl = np.zeros(66, np.uint8)
    nl[0], nl[63], nl[65] = 2, 1, 5
    lay = _hand_layers(66, 2)
    pk = fc.packed_region(nl, 2, lay)
    assert pk.size == 66 * 2 * LAYER
    assert _entry_set(pk.must) == {0, 1, 2, 128, 129}
    assert _entry_set(pk.free) == set(range(132)) - {0, 1, 2, 128, 129}
    e = pk.expect.view(abi.LAYER_DTYPE)
    assert [int(e["offset"][k]) for k in (0, 1, 2, 128, 129)] == [1000, 1001, 1000 + 16 * 63, 1000 + 16 * 65,
                                                                 1001 + 16 * 65]
    assert int(pk.free.sum()) == fc.unspecified_bytes(nl, 2) == 8 * (132 - 5)
    # and the product's position helper agrees with the restated layout
    assert list(abi.packed_positions(nl, 2)[[0, 63, 64, 65]]) == [0, 2, 128, 128]


# ------------------------------------------------------------------ CPU: the classifier against injected faults
def standin(reg: Region, fill: int, zero_free: bool = True) -> np.ndarray:
    """A numpy stand-in for the kernel: the restatement's bytes copied where the footprint says "written"; the
    unspecified bytes zero-filled (as the fast path's whole-row stores do) or left alone."""
    a = np.full(2 * GUARD + reg.size, fill, np.uint8)
    pay = a[GUARD:GUARD + reg.size]
    pay[reg.must] = reg.expect[reg.must]
    if zero_free:
        pay[reg.free] = 0
    return a


def both(reg: Region, fault=None, **kw):
    runs = [standin(reg, f, **kw) for f in FILLS]
    if fault is not None:
        for a, f in zip(runs, FILLS):
            fault(a, a[GUARD:GUARD + reg.size], f)
    return runs


STANDIN_ROW = fc.Row(129, "overflow", 3, True, abi.WINDOW_DEFAULT, F, "all")


def _standin_regions(layout: int) -> dict[str, Region]:
    return fc.expected(replace(STANDIN_ROW, layout=layout))


@pytest.mark.parametrize("layout", [F, P], ids=["fixed", "packed"])
@pytest.mark.parametrize("zero_free", [True, False], ids=["zero_tails", "bare_chains"])
def test_classifier_passes_the_clean_copy(layout, zero_free):
    for reg in _standin_regions(layout).values():
        fc.check(reg, both(reg, zero_free=zero_free))
    st = fc.stats_region(fc.restated(129, "overflow", 3, True)[0])
    runs = []
    for f in FILLS:
        a = np.full(2 * GUARD + st.size, f, np.uint8)
        a[GUARD:GUARD + st.size] = st.expect
        runs.append(a)
    fc.check(st, runs)


def _expect_fault(reg: Region, fault, kinds) -> None:
    with pytest.raises(FootprintError) as e:
        fc.check(reg, both(reg, fault))
    assert e.value.kind in kinds, e.value


def test_classifier_catches_a_record_past_n():
    reg = _standin_regions(F)["summary"]

    def fault(a, pay, fill):  # record n written behind the array (a dead lane of the last tile)
        a[GUARD + reg.size:GUARD + reg.size + 32] = reg.expect[-32:]
    _expect_fault(reg, fault, {"stray write"})


def test_classifier_catches_a_layer_entry_past_the_array():
    for layout in (F, P):
        reg = _standin_regions(layout)["layers"]

        def fault(a, pay, fill):  # entry n * max_layers (an overflowing chain on the last packet)
            a[GUARD + reg.size:GUARD + reg.size + LAYER] = 0x11
        _expect_fault(reg, fault, {"stray write"})


def test_classifier_catches_a_store_into_the_front_guard():
    for name, reg in _standin_regions(F).items():
        def fault(a, pay, fill):
            a[GUARD - 4:GUARD] = 0
        _expect_fault(reg, fault, {"stray write"})


def test_classifier_catches_a_skipped_store_of_a_fill_valued_field():
    # a field whose value is one of the two fills: with that fill alone the skipped store would be invisible
    summary = fc.restated(129, "overflow", 3, True)[0].copy()
    for fill in FILLS:
        summary["hash5"][7] = fill * 0x01010101
        reg = fc.records_region("summary", summary)
        fc.check(reg, both(reg))

        def fault(a, pay, f):
            pay[7 * 32:7 * 32 + 4] = f  # never stored: the bytes keep the run's fill
        _expect_fault(reg, fault, {"missing store"})


def test_classifier_catches_a_skipped_store_of_a_zero_field():
    regs = _standin_regions(F)
    summary = fc.restated(129, "overflow", 3, True)[0]
    i = int(np.nonzero(summary["hash5"] == 0)[0][0])  # hash5 of a packet without a 5-tuple
    for name, at in (("summary", i * 32), ("brief", i * 16), ("flow_keys", i * 4), ("tuples", i * 48 + 40)):
        reg = regs[name]
        assert not reg.expect[at:at + 4].any()

        def fault(a, pay, f):
            pay[at:at + 4] = f
        _expect_fault(reg, fault, {"missing store"})
    # the twelve zero bytes behind an IPv4 address in a pcppx_tuple, and its reserved byte
    tuples = fc.restated(129, "overflow", 3, True)[2]
    j = int(np.nonzero(tuples["ip_version"] == 4)[0][0])
    for at, ln in ((j * 48 + 4, 12), (j * 48 + 47, 1)):
        assert not regs["tuples"].expect[at:at + ln].any()

        def fault(a, pay, f):
            pay[at:at + ln] = f
        _expect_fault(regs["tuples"], fault, {"missing store"})


def test_classifier_catches_a_packed_run_shifted_by_one_entry():
    reg = _standin_regions(P)["layers"]

    def fault(a, pay, fill):
        run = np.nonzero(reg.must[:64 * 3 * LAYER])[0]
        lo, hi = int(run[0]), int(run[-1]) + 1
        pay[lo + LAYER:hi + LAYER] = reg.expect[lo:hi]
        pay[lo:lo + LAYER] = fill
    _expect_fault(reg, fault, {"missing store", "wrong value"})


def test_classifier_catches_a_packed_write_into_the_next_tiles_region():
    reg = _standin_regions(P)["layers"]
    at = 64 * 3 * LAYER  # tile 1's region starts here, with its first chain's first entry
    assert reg.must[at:at + LAYER].all()

    def fault(a, pay, fill):  # tile 0's run spills one entry over its region's end
        pay[at:at + LAYER] = reg.expect[at - 64 * 3 * LAYER:at - 64 * 3 * LAYER + LAYER] ^ 0x80
    _expect_fault(reg, fault, {"wrong value"})


def test_classifier_catches_a_byte_that_differs_between_the_runs():
    reg = _standin_regions(F)["summary"]
    with pytest.raises(FootprintError) as e:
        runs = both(reg)
        runs[1][GUARD + 40] ^= 1
        fc.check(reg, runs)
    assert e.value.kind in ("not deterministic", "wrong value")


# ------------------------------------------------------------------ CPU: the table and the batches
def test_table_covers_every_axis_value():
    assert fc.check_table() == []
    assert len(fc.TABLE) <= 120  # pairwise, not the cross product
    # the checker itself can fail: a table without its PACKED rows, or without one n, is refused
    assert fc.check_table(tuple(r for r in fc.TABLE if r.layout != P))
    assert fc.check_table(tuple(r for r in fc.TABLE if r.n != 4097))
    assert fc.check_table(tuple(r for r in fc.TABLE if not (r.ml == 12 and r.window == abi.WINDOW_SHORT)))


def test_batches_hold_what_the_footprint_needs():
    L = len(fc.mixed_list())
    s, lay, tup = fc.restated(L, "fast", 16, True)
    fl = s["flags"]
    # fast-path shapes, generic-walk shapes, stacks deeper than 3, 5, 8 and 12 layers (and one deeper than 16)
    for depth in (3, 5, 8, 12):
        assert int((s["n_layers"] > depth).sum()) >= 2, depth
    assert bool((fl & abi.F_DEPTH_OVERFLOW).any())
    # the edge descriptors: empty and 1-B packets, the oversize packet, the descriptor past data_len
    b = fc.batch(L, "fast")
    assert 0 in b.caplens and 1 in b.caplens and fc.OVERSIZE in b.caplens
    assert bool((fl & abi.F_OVERSIZE).any()) and bool((fl & abi.F_BAD_DESC).any())
    assert int(b.offsets.max()) + 60 > len(b.data)
    # the values a missing store hides behind zero-filled outputs: hash5 0, flags 0, n_layers 0, IPv4 tuples
    assert bool((s["hash5"] == 0).any()) and bool((s["hash5"] != 0).any())
    assert bool((fl == 0).any()) and bool((s["n_layers"] == 0).any()) and bool((tup["ip_version"] == 4).any())
    assert bool((fl & abi.F_NEEDS_HOST_L7).any()) and bool((fl & abi.F_L7_KNOWN).any())
    # each rotation puts its packet last, at every n
    for n in fc.NS:
        for ml in (3, 16):
            s, _, _ = fc.restated(n, "fast", ml, False)
            assert int(s["flags"][-1]) & abi.F_NEEDS_HOST == 0 and int(s["n_layers"][-1]) == min(4, ml) \
                and int(s["hash5"][-1]) != 0  # Ethernet, IPv4, UDP, payload
            s, _, _ = fc.restated(n, "overflow", ml, False)
            assert int(s["flags"][-1]) & abi.F_DEPTH_OVERFLOW and int(s["n_layers"][-1]) == ml
            s, _, _ = fc.restated(n, "unparsed", ml, False)
            assert int(s["flags"][-1]) & abi.F_BAD_DESC and int(s["n_layers"][-1]) == 0
    # the stale-buffer test's second batch: shorter chains and other flags, packet by packet
    for n in (129, 4097):
        a, _, _ = fc.restated(n, "overflow", 8, True)
        bb, _ = oracle.oracle_parse(fc.stale_batch(n), fc.opts_of(8, True))
        assert int((bb["n_layers"] < a["n_layers"]).sum()) > n // 2
        assert int((bb["flags"] != a["flags"]).sum()) > n // 2


def test_header_states_the_pinned_footprint():
    """include/pcppx.h says what these tests pin: the PACKED region bound, the unspecified rest of it, the rows of
    FIXED, and the natural alignment of the record arrays."""
    text = " ".join((abi.REPO_DIR / "include" / "pcppx.h").read_text().replace("*", " ").split())
    for phrase in ("A tile writes only inside its own region, entries [64 t max_layers, min(64 (t + 1), n) max_layers)",
                   "the rest of the region is unspecified", "Nothing is written at or past layers[n max_layers]",
                   "Nothing is written outside rows 0 .. n-1", "every array must have its record's natural alignment",
                   "16 bytes for summary, brief, tuples and pcppx_reasm_info, 8 bytes for layers and proto_stats, 4 bytes "
                   "for flow_keys"):
        assert phrase in text, phrase
    assert "only the chain's entries are written" not in text


# ------------------------------------------------------------------ consumers ignore unspecified entries
# The named subsets: each operator's smallest cases that hold flagged, overflowing and zero-layer packets (where its
# case list has them), a case per record kind (summary / brief) and per max_layers it runs with.
CONSUMERS = {
    "defrag": (defrag_cases, ("mixed", "n1_fragment", "g3_shuffled", "total_65515")),
    "defrag6": (defrag6_cases, ("n1_fragment", "g3_shuffled", "hbh_ahead", "swap_0800")),
    "frag": (frag_cases, ("bad_records", "dispositions_df0", "trailer", "cut_capture")),
    "frag6": (frag6_cases, ("plain", "vlan1", "hbh_routing_dst", "ah_24_behind_hbh")),
    "tcpstream": (tcpstream_cases, ("n1_data", "tcp_options", "ooo_alone_bc1", "trailer")),
    "tlsfp": (tlsfp_cases, ("flags", "flags_brief", "max_layers_4", "text_lengths")),
    "dns": (dns_cases, ("flags", "records", "max_layers_3", "parsed_ml3")),
    "http": (http_cases, ("flags", "records", "max_layers_4", "max_layers_16")),
}
# The case lists of the operators that move packets hold no overflowing or zero-layer packet (their records are parses
# of well-formed stacks at max_layers 6), so each of them also runs over the footprint mix: stacks deeper than 6 layers
# (PCPPX_F_DEPTH_OVERFLOW), empty and 1-B packets (n_layers 0 / 1), flagged L7 payloads, and IPv4 / IPv6 fragments and
# TCP segments for them to work on.
MIX = "footprint_mix"
MIX_KW = {"defrag": {}, "defrag6": {}, "frag": {"frag_size": 64}, "frag6": {"frag_size": 64}, "tcpstream": {}}
CONSUMER_IDS = [f"{op}-{name}" for op, (_, names) in CONSUMERS.items() for name in names] + [f"{op}-{MIX}" for op in MIX_KW]


def mix_packets() -> list[bytes]:
    import mutate

    return [p for p in fc.mixed_list() if isinstance(p, bytes)] + [b"", b"\x77"] + mutate.fragments(120)


@pytest.fixture(scope="module")
def consumer_cases():
    out = {}
    for op, (mod, names) in CONSUMERS.items():
        by_name = {c.name: c for c in mod.cases()}
        for name in names:
            out[f"{op}-{name}"] = (mod, by_name[name])
        if op in MIX_KW:
            out[f"{op}-{MIX}"] = (mod, mod.make(MIX, mix_packets(), **MIX_KW[op]))
    return out


def _poisoned_case(c):
    lay = fc.poisoned(c.layers, c.summary["n_layers"])
    ml = c.layers.shape[1]
    changed = int((lay.view(np.uint8) != np.ascontiguousarray(c.layers).view(np.uint8)).sum())
    free = int((ml - fc.chain_counts(c.summary["n_layers"], ml)).sum())
    assert (changed > 0) == (free > 0)
    return replace(c, layers=lay), free


SAME = {defrag6_cases: defrag_cases.assert_same, frag6_cases: frag_cases.assert_same}  # the modules they extend


def _same_buffers(mod, got, want, what):
    """Whole buffers, pads included, and the totals (each operator's own assert_same)."""
    (SAME.get(mod) or mod.assert_same)(got, want, what)


@pytest.mark.parametrize("which", CONSUMER_IDS)
def test_reference_consumers_ignore_unspecified_entries(consumer_cases, which):
    mod, c = consumer_cases[which]
    bad, _ = _poisoned_case(c)
    _same_buffers(mod, mod.run_reference(bad), mod.run_reference(c), which)


def test_consumer_subsets_hold_unspecified_entries():
    """The subsets are worth running: every operator sees entries past a chain, and the ones whose case lists have
    them see flagged, overflowing and zero-layer packets."""
    seen = {}
    for op, (mod, names) in CONSUMERS.items():
        by_name = {c.name: c for c in mod.cases()}
        free = flagged = over = zero = 0
        for c in [by_name[name] for name in names] + ([mod.make(MIX, mix_packets(), **MIX_KW[op])] if op in MIX_KW else []):
            free += _poisoned_case(c)[1]
            flagged += int(((c.summary["flags"] & abi.F_NEEDS_HOST) != 0).sum())
            over += int(((c.summary["flags"] & abi.F_DEPTH_OVERFLOW) != 0).sum())
            zero += int((c.summary["n_layers"] == 0).sum())
        seen[op] = (free, flagged, over, zero)
        assert free > 0, op
    for op in CONSUMERS:
        assert all(v > 0 for v in seen[op]), (op, seen[op])


def _record_cases(n: int = 300):
    """select in flags mode and steer by hash5 over a parse's records: the summary (or brief) is their whole input."""
    b = fc.batch(n, "overflow")
    summary, layers, _ = fc.restated(n, "overflow", 6, True)
    out = []
    for rec in (summary, fc.brief_of(summary)):
        raw = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)
        out.append((select_cases, select_cases.Case(f"select_flags_{rec.dtype.itemsize}", b.data, b.offsets, b.caplens,
                                                     keep=None, flags=raw, flags_stride=rec.dtype.itemsize,
                                                     flags_any=abi.F_NEEDS_HOST | abi.F_DEPTH_OVERFLOW)))
        out.append((steer_cases, steer_cases.Case(f"steer_hash5_{rec.dtype.itemsize}", b.data, b.offsets, b.caplens,
                                                   n_buckets=7, bucket=None, key=raw, key_stride=rec.dtype.itemsize,
                                                   key_offset=0)))
    return out, summary, layers


def test_select_and_steer_read_no_layer_entries():
    """pcppx_select_device in flags mode and pcppx_steer_device by hash5 take the summary or the brief alone: a record
    set whose unspecified layer entries are poisoned is, to them, the same input. Run both ways all the same, so that
    the day one of them is handed the layers it is covered here."""
    cases, summary, layers = _record_cases()
    assert fc.poisoned(layers, summary["n_layers"]).tobytes() != layers.tobytes()
    for mod, c in cases:
        want = mod.run_reference(c)
        mod.assert_same(mod.run_reference(replace(c)), want, c.name)
        mod.assert_same(mod.brute(c), want, c.name)


# ------------------------------------------------------------------ GPU: the table through the device parse
_DEV = {}


def _device_batch(n: int, rotation: str):
    if (n, rotation) not in _DEV:
        _DEV[(n, rotation)] = fc.device_batch(fc.batch(n, rotation))
    return _DEV[(n, rotation)]


@pytest.fixture(scope="module")
def engines():
    """Two contexts: one sees the table with n ascending, the other with n descending."""
    from pcapplusplus_amd.engine import Engine

    e = {"ascending": Engine(0), "descending": Engine(0)}
    yield e
    for x in e.values():
        x.close()
    _DEV.clear()


ORDERED = [("ascending", r) for r in sorted(fc.TABLE, key=lambda r: r.n)] + \
          [("descending", r) for r in sorted(fc.TABLE, key=lambda r: -r.n)]


def _check_all(regions: dict, runs: list) -> None:
    for name, reg in regions.items():
        fc.check(reg, (runs[0][name], runs[1][name]))


@pytest.mark.gpu
@pytest.mark.parametrize("order,row", ORDERED, ids=[f"{o}-{r.id}" for o, r in ORDERED])
def test_gpu_parse_footprint(engines, order, row):
    regions = fc.expected(row)
    dev = _device_batch(row.n, row.rotation)
    runs = [fc.device_parse(engines[order], dev, row, regions, fill) for fill in FILLS]
    _check_all(regions, runs)


@pytest.mark.gpu
@pytest.mark.parametrize("ml", [8, 16])
@pytest.mark.parametrize("n", [63, 64, 65, 4097])
def test_gpu_parse_reasm_footprint(engine, n, ml):
    """pcppx_parse_batch_device_reasm: info[0..n) written and equal to pcppx_reasm_device over the restatement's
    records, the rest untouched; the records as in a plain parse."""
    import torch

    rotation = fc.ROTATIONS[fc.NS.index(n) % 3]
    summary, layers, _ = fc.restated(n, rotation, ml, True)
    data, offsets, caplens = _device_batch(n, rotation)
    stream = torch.cuda.current_stream("cuda:0").cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
    info_t = torch.zeros(n * 16, dtype=torch.uint8, device="cuda:0")
    engine.reasm_device(data, offsets, caplens, n, 1, up(summary), up(layers), ml, info_t, stream)
    torch.cuda.synchronize()
    info = info_t.cpu().numpy().view(abi.REASM_DTYPE)
    regions = {"summary": fc.records_region("summary", summary), "layers": fc.fixed_region(summary["n_layers"], ml, layers),
               "info": fc.records_region("info", info)}
    assert int(regions["layers"].free.sum()) == fc.unspecified_bytes(summary["n_layers"], ml)
    runs = []
    for fill in FILLS:
        ar = fc.DeviceArenas(regions, fill)
        engine.parse_reasm_device(data, offsets, caplens, n, 1, fc.opts_of(ml, True), ar.out("summary"),
                                  ar.out("layers"), ar.out("info"), stream)
        torch.cuda.synchronize()
        runs.append(ar.host())
    _check_all(regions, runs)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("layout", [abi.LAYOUT_FIXED, abi.LAYOUT_DENSE], ids=["fixed", "dense"])
@pytest.mark.parametrize("n", fc.NS)
def test_gpu_host_parse_footprint(engine, n, layout, pinned):
    """pcppx_parse_batch_host into guarded numpy arenas: FIXED as on the device; DENSE: the chains back to back, every
    byte past them untouched, layers_written the restatement's total."""
    k = fc.NS.index(n)
    ml = (1, 3, 8, 12, 16, 5, 13, 2, 16, 11)[k]
    rotation = fc.ROTATIONS[(k + (layout == abi.LAYOUT_DENSE)) % 3]
    csum = bool(k & 1)
    outputs = ("summary", "brief", "both")[(k + pinned) % 3]
    summary, layers, _ = fc.restated(n, rotation, ml, csum)
    regions = {}
    if outputs in ("summary", "both"):
        regions["summary"] = fc.records_region("summary", summary)
    if outputs in ("brief", "both"):
        regions["brief"] = fc.records_region("brief", fc.brief_of(summary))
    if layout == abi.LAYOUT_DENSE:
        regions["layers"], written = fc.dense_region(summary["n_layers"], ml, layers)
        assert written == int(fc.chain_counts(summary["n_layers"], ml).sum())
    else:
        regions["layers"], written = fc.fixed_region(summary["n_layers"], ml, layers), n * ml
        assert int(regions["layers"].free.sum()) == fc.unspecified_bytes(summary["n_layers"], ml)
    runs = []
    for fill in FILLS:
        got, w = fc.host_parse(engine, fc.batch(n, rotation), fc.opts_of(ml, csum, layout=layout), regions, fill, pinned)
        assert w == written, (w, written)
        runs.append(got)
    _check_all(regions, runs)


@pytest.mark.gpu
@pytest.mark.parametrize("records", ["summary", "brief"])
@pytest.mark.parametrize("layout", [F, P], ids=["fixed", "packed"])
@pytest.mark.parametrize("n", [129, 4097])
def test_gpu_stale_buffers_decode(engine, n, layout, records):
    """Batch A, then a different batch B of the same n (shorter chains, other flags) parsed into the same, never
    filled buffers, as a caller that reuses its buffers does: the decoded records of B are the restatement's."""
    import torch

    ml = 8
    opts = fc.opts_of(ml, True, layout=layout)
    stream = torch.cuda.current_stream("cuda:0").cuda_stream
    rec_t = torch.empty(n * (32 if records == "summary" else 16), dtype=torch.uint8, device="cuda:0")
    lay_t = torch.empty(n * ml * LAYER, dtype=torch.uint8, device="cuda:0")
    fk_t = torch.empty(n, dtype=torch.int32, device="cuda:0")
    tp_t = torch.empty(n * 48, dtype=torch.uint8, device="cuda:0")
    for b in (fc.batch(n, "overflow"), fc.stale_batch(n)):
        data, offsets, caplens = fc.device_batch(b)
        engine.parse_device(data, offsets, caplens, n, 1, opts, rec_t if records == "summary" else None, lay_t, stream,
                            flow_keys=fk_t, tuples=tp_t, brief=rec_t if records == "brief" else None)
        torch.cuda.synchronize()
    want_s, want_l, want_t = oracle.oracle_parse_tuples(fc.stale_batch(n), fc.opts_of(ml, True))
    want_r = want_s if records == "summary" else fc.brief_of(want_s)
    got_r = rec_t.cpu().numpy().view(want_r.dtype)
    assert got_r.tobytes() == want_r.tobytes()
    assert fk_t.cpu().numpy().view(np.uint32).tobytes() == want_s["hash5"].tobytes()
    assert tp_t.cpu().numpy().tobytes() == want_t.tobytes()
    raw = np.ascontiguousarray(lay_t.cpu().numpy()).view(abi.LAYER_DTYPE)
    if layout == P:
        fixed = np.full((n, ml), 0x33, np.uint8).repeat(LAYER, axis=1).view(abi.LAYER_DTYPE).copy()
        call = engine.lib.pcppx_unpack_layers if records == "summary" else engine.lib.pcppx_unpack_layers_brief
        abi.check(call(got_r.ctypes.data, raw.ctypes.data, n, ml, fixed.ctypes.data), "pcppx_unpack_layers")
        assert fixed.tobytes() == want_l.tobytes()  # zero past each chain: the decoder's contract
    else:
        chain = np.arange(ml)[None, :] < fc.chain_counts(want_s["n_layers"], ml)[:, None]
        assert raw.reshape(n, ml)[chain].tobytes() == want_l[chain].tobytes()


# ------------------------------------------------------------------ GPU: consumers over poisoned records
@pytest.mark.gpu
@pytest.mark.parametrize("which", CONSUMER_IDS)
def test_gpu_consumers_ignore_unspecified_entries(engine, consumer_cases, which):
    mod, c = consumer_cases[which]
    bad, _ = _poisoned_case(c)
    want = mod.run_device(engine, c)
    _same_buffers(mod, mod.run_device(engine, bad), want, which)
    _same_buffers(mod, want, mod.run_reference(c), which)


@pytest.mark.gpu
def test_gpu_select_and_steer_read_no_layer_entries(engine):
    for mod, c in _record_cases()[0]:
        mod.assert_same(mod.run_device(engine, c), mod.run_reference(c), c.name)


@pytest.mark.gpu
@pytest.mark.parametrize("ml", [6, 16])
def test_gpu_filter_and_reasm_ignore_unspecified_entries(engine, ml):
    """pcppx_filter_device and pcppx_reasm_device have no CPU reference: the run over the clean records (zero past
    each chain) is the expectation for the run over the poisoned ones."""
    import torch

    n = 700
    b = fc.batch(n, "overflow")
    summary, layers, _ = fc.restated(n, "overflow", ml, True)
    bad = fc.poisoned(layers, summary["n_layers"])
    assert bad.tobytes() != layers.tobytes()
    data, offsets, caplens = fc.device_batch(b)
    stream = torch.cuda.current_stream("cuda:0").cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda:0")  # noqa: E731
    sum_t = up(summary)
    spec = oracle.make_spec(src_ip="10.1.2.3", dst_port=50000, protocol=oracle.P_UDP)
    got = []
    for lay in (layers, bad):
        lay_t = up(lay)
        info = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda:0")
        engine.reasm_device(data, offsets, caplens, n, 1, sum_t, lay_t, ml, info, stream)
        keys = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
        first = torch.zeros(4096, dtype=torch.int64, device="cuda:0")
        matched = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
        stats = torch.zeros(len(abi.STATS_FIELDS) + 2, dtype=torch.int64, device="cuda:0")
        engine.filter_device(data, offsets, caplens, n, 1, sum_t, lay_t, ml, spec, 0, keys, first, 4096, matched, stats,
                             stream)
        torch.cuda.synchronize()
        got.append([t.cpu().numpy().tobytes() for t in (info, keys, first, matched, stats)])
    assert got[0][3].count(1) > 0  # the spec matches some packets: the filter did read the layers
    for x, y, what in zip(got[0], got[1], ("reasm info", "flow keys", "flow first", "matched", "stats")):
        assert x == y, what
    want = oracle.oracle_reasm(b, summary, layers)
    assert got[0][0] == want.tobytes()
