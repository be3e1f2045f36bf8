"""Every decoder of the parse slid across the edges of the header windows (tests/window_cases.py).

The tile kernel reads headers through an LDS window of 96, 128 or 144 B minus the packet's start alignment; at or past
the window's end the guarded readers fall back to HBM bytes, and any of fast_walk's `... <= p.lim` conditions sends a
packet to the generic walk, which must give bit-identical records. The rest of the suite reaches those bytes by chance
(L7 text aside); here the grid enumerates them: every header kind at every distance from -h - 1 to +1 of every edge
(the re-gathered window included), cut at every byte of the header, in three tile compositions, through the four
product instances and every output set.

CPU: the grid's reach, its checksum share, and the restatement over it against the reference Packet++ (live where it is
built, and always against the frozen tests/golden/window/grid.npz). GPU: the engine's records, tuples, flow keys,
PACKED rows and fused reassembly info against the restatement, the frozen reference records, the lane cross-check
kernel, and the fast path's share of the grid.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

import oracle
import window_cases as wc
from conftest import GOLDEN, load_golden
from pcapplusplus_amd import abi

FIXTURE = GOLDEN / "window" / "grid.npz"
CSUM_BITS = abi.F_IP_CSUM | abi.F_IP_CSUM_OK | abi.F_L4_CSUM | abi.F_L4_CSUM_OK
CSUM_FIELDS = ("ip_csum_calc", "ip_csum_stored", "l4_csum_calc", "l4_csum_stored")
FAST_MARK = 0x8000  # tools/ab variants 30 / 31: flags bit on the packets the fast path took


# ---------------------------------------------------------------- shared, computed once
@lru_cache(maxsize=None)
def distinct():
    return wc.distinct_batch()


@lru_cache(maxsize=None)
def golden():
    """(batch, {variant: (opts, reference summary, reference layers)}) of the frozen fixture."""
    return load_golden(FIXTURE)


@lru_cache(maxsize=None)
def restated_distinct(variant: str):
    opts = golden()[1][variant][0]
    return oracle.oracle_parse(distinct(), opts)


@lru_cache(maxsize=None)
def restated(comp: str, csum: bool, ml: int):
    """The restatement's (summary, layers, tuples) of a composition (the window is a speed choice: no part of it)."""
    return oracle.oracle_parse_tuples(wc.placed(comp).batch, abi.make_opts(0, 8, csum, ml))


def without_checksums(rsum: np.ndarray) -> np.ndarray:
    """Reference summaries as a parse-only launch reports them: no checksum fields, no verdict bits."""
    out = rsum.copy()
    out["flags"] &= ~np.uint16(CSUM_BITS)
    for f in CSUM_FIELDS:
        out[f] = 0
    return out


def reference_rows(variant: str, uid: np.ndarray, csum: bool):
    _, variants = golden()
    _, rsum, rlay = variants[variant]
    rows = wc.fixture_rows(uid)
    rsum = rsum[rows]
    return (rsum if csum else without_checksums(rsum)), rlay[rows]


# ---------------------------------------------------------------- CPU: the generator
def test_window_constants_and_instances():
    """The four instances' windows as the kernel source states them; the grid below is built for these edges."""
    inst = wc.instances()
    assert [(i.first, i.full) for i in inst.values()] == [(96, 96), (96, 144), (128, 144), (96, 96)], inst
    assert wc.edges() == (96, 128, 144)
    for comp in wc.COMPOSITIONS:
        pl = wc.placed(comp)
        assert pl.batch.n <= wc.MAX_DESCRIPTORS
        tiles = pl.slid[: pl.batch.n // wc.TILE * wc.TILE].reshape(-1, wc.TILE).sum(axis=1)
        want = {"solid": wc.TILE, "mixed": wc.TILE // 2, "lone": 1}[comp]
        assert (tiles == want).all(), (comp, np.unique(tiles))
    assert 1000 <= len(wc.grid()) <= 6000


def test_grid_reach():
    """For every header kind (start s, length h, both checked against the restatement's layer records) and every edge E
    of a window of E - mis bytes, mis = address mod 16: the distances s - (E - mis) over the grid hold every integer in
    [-h - 1, +1]; the same for the re-gathered 144-B window (mis = address mod 4, packets long enough to take it:
    (mis + caplen) >> 4 >= Chunks); and the cut packets' caplen - s hold every integer in [-1, h + 1]."""
    g = wc.grid()
    osum, olay = restated_distinct("full")
    regather = wc.regather_edge()
    dist = {k: {e: set() for e in wc.edges()} for k in wc.KINDS}
    redist = {k: set() for k in wc.KINDS}
    cuts = {k: set() for k in wc.KINDS}
    hs = {}
    uncut = {(sl.kind, sl.flavor, sl.s) for sl in g if sl.mode != "cut"}
    for u, sl in enumerate(g):
        kind = wc.KINDS[sl.kind]
        if sl.mode == "cut":
            assert (sl.kind, sl.flavor, sl.s) in uncut and all(-2 <= sl.s - (e - a) <= 8 for a in sl.aligns
                                                               for e in wc.edges() if e - 4 < sl.s <= e), sl
            cuts[sl.kind].add(sl.caplen - sl.s)
            continue
        lay = olay[u][: int(osum["n_layers"][u])]
        at = np.nonzero((lay["offset"] == sl.s) & (lay["proto"] == kind.proto))[0]
        assert len(at) == 1, f"{sl.kind} {sl.flavor} s={sl.s}: no layer {kind.proto} at s in {lay}"
        h = int(lay["hdr_len"][at[0]]) if kind.whole else kind.h
        assert h == kind.h and hs.setdefault(sl.kind, h) == h, (sl.kind, sl.flavor, sl.s, h, kind.h)
        for a in sl.aligns:
            for e in wc.edges():
                dist[sl.kind][e].add(sl.s - (e - a))
            if (a % 4 + sl.caplen) >> 4 >= regather // 16:
                redist[sl.kind].add(sl.s - (regather - a % 4))
    miss = []
    for k, kind in wc.KINDS.items():
        want = set(range(-kind.h - 1, 2))
        for e in wc.edges():
            if want - dist[k][e]:
                miss.append(f"{k} edge {e}: {sorted(want - dist[k][e])}")
        if want - redist[k]:
            miss.append(f"{k} re-gathered {regather}: {sorted(want - redist[k])}")
        if set(range(-1, kind.h + 2)) - cuts[k]:
            miss.append(f"{k} cuts: {sorted(set(range(-1, kind.h + 2)) - cuts[k])}")
    assert not miss, "\n".join(miss)


def test_grid_placements():
    """Each header kind at least once as the first layer behind padding that adds no layer record (outermost behind
    VLAN tags, or behind one IP header with options / an extension) and once as an inner layer behind a tunnel (IPIP,
    6in4, 4in6, GRE, VXLAN, GTP); every padding brick occurs."""
    osum, olay = restated_distinct("full")
    tunnel = {k: False for k in wc.KINDS}
    first = {k: False for k in wc.KINDS}
    for u, sl in enumerate(wc.grid()):
        if sl.mode == "cut":
            continue
        lay = olay[u][: int(osum["n_layers"][u])]
        before = [int(p) for p in lay["proto"][lay["offset"] < sl.s]]
        ips = sum(p in (2, 3) for p in before)
        tunnel[sl.kind] |= ips >= 2 or any(p in (15, 16, 26, 32) for p in before)
        first[sl.kind] |= ips <= 1 and not any(p in (15, 16) for p in before)
    assert all(tunnel.values()) and all(first.values()), (tunnel, first)
    flavors = {sl.flavor for sl in wc.grid()}
    assert flavors == {"outer", "fast4", "v4", "v6", "fast4+gre", "v4+gre", "v6+gre"}, flavors


def test_grid_checksum_share():
    """At least half of the packets with an L4 layer verify (F_L4_CSUM_OK in the restatement's records), at least a
    tenth do not; a flipped bit flips exactly its verdict, and no unflipped packet fails one."""
    osum, _ = restated_distinct("full")
    fl = osum["flags"][: len(wc.grid())]
    l4 = (fl & abi.F_L4_CSUM) != 0
    ok = (fl & abi.F_L4_CSUM_OK) != 0
    ip, ipok = (fl & abi.F_IP_CSUM) != 0, (fl & abi.F_IP_CSUM_OK) != 0
    assert l4.sum() >= 1000 and ok[l4].mean() >= 0.5 and (~ok[l4]).mean() >= 0.1, (int(l4.sum()), float(ok[l4].mean()))
    flip = np.array([{None: 0, "l4": 1, "ip": 2}[sl.flip] for sl in wc.grid()])
    assert (ok[l4] == (flip[l4] != 1)).all()
    # the IPv4 verdict likewise, where the first IPv4 header is captured whole (a cut through its options leaves a
    # header that cannot verify, flipped or not)
    whole = ip & np.array([sl.mode != "cut" for sl in wc.grid()])
    assert (ipok[whole] == (flip[whole] != 2)).all() and not (ipok & (flip == 2)).any()
    assert (~ipok[whole]).sum() >= 100


# ---------------------------------------------------------------- CPU: restatement against reference
def check_against_reference(batch, opts, rsum, rlay) -> dict:
    osum, olay = oracle.oracle_parse(batch, opts)
    st = oracle.compare_engine_to_reference(osum, olay, rsum, rlay)
    st.update(oracle.check_flag_contract(osum, rsum, rlay, batch))
    return st


def test_fixture_is_the_grid():
    """Regenerating the packets gives the fixture's bytes (the grid is a pure function of the window sizes)."""
    b, variants = golden()
    d = distinct()
    assert set(variants) == {"full", "until_tcp", "ml5"}
    assert np.array_equal(b.offsets, d.offsets) and np.array_equal(b.caplens, d.caplens)
    assert b.data.tobytes() == d.data.tobytes()
    assert list(b.meta["set_names"]) == list(wc.KINDS) + ["plain"]
    assert FIXTURE.stat().st_size < 1_000_000


@pytest.mark.parametrize("variant", ["full", "until_tcp", "ml5"])
def test_restatement_matches_frozen_reference(variant):
    b, variants = golden()
    opts, rsum, rlay = variants[variant]
    st = check_against_reference(b, opts, rsum, rlay)
    assert st["n"] == len(wc.grid()) + len(wc.PLAIN) and st["exact"] >= st["n"] // 2, st
    # a parse-only launch: the same records without the checksum fields and verdict bits
    po = abi.make_opts(opts.parse_until_family, opts.parse_until_osi, False, opts.max_layers)
    check_against_reference(b, po, without_checksums(rsum), rlay)


@pytest.mark.skipif(not oracle.ref_available(), reason="reference Packet++ not built here (oracle/_ref)")
@pytest.mark.parametrize("variant", ["full", "until_tcp", "ml5"])
def test_restatement_matches_live_reference(variant):
    b, variants = golden()
    opts, rsum, rlay = variants[variant]
    live = oracle.ref_parse(distinct(), opts)
    oracle.compare_exact(live[0], live[1], rsum, rlay)  # the frozen records are the reference's
    check_against_reference(distinct(), opts, live[0], live[1])
    for comp in wc.COMPOSITIONS:  # and over the placed descriptors (every alignment; shared bytes)
        pb = wc.placed(comp).batch
        check_against_reference(pb, opts, *oracle.ref_parse(pb, opts))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def fresh_engines():
    """One fresh Engine per instance: every launch forces its window, so WINDOW_DEFAULT resolution never enters."""
    from pcapplusplus_amd.engine import Engine

    made = {}

    def get(name: str):
        if name not in made:
            made[name] = Engine(0)
        return made[name]

    yield get
    for e in made.values():
        e.close()


_device: dict[str, tuple] = {}


def device_batch(comp: str):
    from pcapplusplus_amd.engine import to_device

    if comp not in _device:
        _device[comp] = to_device(wc.placed(comp).batch)
        assert _device[comp][0].data_ptr() % 16 == 0  # a packet's offset mod 16 is its address mod 16
    return _device[comp]


def device_parse(eng, comp: str, opts: abi.Opts, *, tuples=False, flow_keys=False, reasm=False, variant=None) -> dict:
    """One launch over a composition: the product's parse, the fused parse + reassembly pass (reasm), or a tools/ab
    variant. Returns summary / layers (FIXED rows; PACKED rows unpacked) / tuples / flow_keys / info."""
    import torch

    data, offsets, caplens = device_batch(comp)
    n, ml = wc.placed(comp).batch.n, opts.max_layers
    dev = data.device
    z = lambda k: torch.zeros(max(k, 1), dtype=torch.uint8, device=dev)  # noqa: E731
    st, lay = z(n * 32), z(n * ml * 8)
    tp = z(n * 48) if tuples else None
    fk = torch.zeros(n, dtype=torch.int32, device=dev) if flow_keys else None
    info = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device=dev) if reasm else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    if variant is not None:
        from tools import ab

        ab.parse_device(data, offsets, caplens, n, 1, opts, st, lay, stream, variant)
    elif reasm:
        eng.parse_reasm_device(data, offsets, caplens, n, 1, opts, st, lay, info, stream)
    else:
        eng.parse_device(data, offsets, caplens, n, 1, opts, st, lay if ml else None, stream, flow_keys=fk, tuples=tp)
    torch.cuda.synchronize(dev)
    out = {"summary": st.cpu().numpy().view(abi.SUMMARY_DTYPE)[:n]}
    raw = lay.cpu().numpy()[: n * ml * 8].view(abi.LAYER_DTYPE)
    out["layers"] = abi.unpack_layers(out["summary"], raw, ml) if opts.layout == abi.LAYOUT_PACKED else raw.reshape(n, ml)
    if tuples:
        out["tuples"] = tp.cpu().numpy().view(abi.TUPLE_DTYPE)[:n]
    if flow_keys:
        out["flow_keys"] = fk.cpu().numpy().view(np.uint32)[:n]
    if reasm:
        out["info"] = info.cpu().numpy().view(abi.REASM_DTYPE)[:n]
    return out


def describe(comp: str, i: int) -> str:
    pl = wc.placed(comp)
    u = int(pl.uid[i])
    if u < 0:
        return f"{comp} #{i}: plain packet, start%16={int(pl.align[i])}"
    sl = wc.grid()[u]
    return (f"{comp} #{i}: {sl.kind} behind {sl.flavor} padding, header at {sl.s} (h={sl.h}), {sl.mode}, caplen "
            f"{sl.caplen}, start%16={int(pl.align[i])}, grid row {u}")


def assert_records(comp: str, got: dict, want, what: str) -> None:
    try:
        oracle.compare_exact(got["summary"], got["layers"], want[0], want[1])
    except AssertionError as e:
        i = int(str(e).split("first #")[1].split(":")[0])
        raise AssertionError(f"{what}: {describe(comp, i)}\n{e}") from None


def assert_equal_fields(a: np.ndarray, b: np.ndarray, comp: str, what: str) -> None:
    for f in (a.dtype.names or (None,)):
        x, y = (a, b) if f is None else (a[f], b[f])
        bad = np.nonzero((x != y).reshape(len(x), -1).any(axis=1))[0]
        assert not len(bad), f"{what}.{f} differs on {len(bad)} packets; first {describe(comp, int(bad[0]))}: " \
                             f"{a[bad[0]]} vs {b[bad[0]]}"


INSTANCES = pytest.mark.parametrize("inst", list(wc.instances()))
COMPS = pytest.mark.parametrize("comp", wc.COMPOSITIONS)


@pytest.mark.gpu
@INSTANCES
@COMPS
def test_gpu_window_grid_records(fresh_engines, inst, comp):
    """FIXED rows with max_layers 16 and 5 and PACKED rows with max_layers 8: every record field equals the
    restatement's; the max_layers 16 and 5 records meet the engine contract against the frozen reference records."""
    I = wc.instances()[inst]
    eng = fresh_engines(inst)
    pl = wc.placed(comp)
    for ml, layout, variant in ((16, abi.LAYOUT_FIXED, "full"), (5, abi.LAYOUT_FIXED, "ml5"), (8, abi.LAYOUT_PACKED, None)):
        g = device_parse(eng, comp, I.opts(ml, layout))
        o = restated(comp, I.csum, ml)
        assert_records(comp, g, o, f"{inst} max_layers {ml} layout {layout}")
        if variant is not None:
            rsum, rlay = reference_rows(variant, pl.uid, I.csum)
            oracle.compare_engine_to_reference(g["summary"], g["layers"], rsum, rlay)
            oracle.check_flag_contract(g["summary"], rsum, rlay, pl.batch)


@pytest.mark.gpu
@INSTANCES
@COMPS
def test_gpu_window_grid_tuples_and_flow_keys(fresh_engines, inst, comp):
    """Summary + 5-tuple extracts + flow keys (no layer rows): the summary and the tuples equal the restatement's, the
    flow keys its hash5."""
    I = wc.instances()[inst]
    g = device_parse(fresh_engines(inst), comp, I.opts(0), tuples=True, flow_keys=True)
    osum, _, otup = restated(comp, I.csum, 0)
    assert_equal_fields(g["summary"], osum, comp, "summary")
    assert_equal_fields(g["tuples"], otup, comp, "tuples")
    assert_equal_fields(g["flow_keys"], osum["hash5"].astype(np.uint32), comp, "flow_keys")


@pytest.mark.gpu
@INSTANCES
@COMPS
def test_gpu_window_grid_fused_reasm(fresh_engines, inst, comp):
    """pcppx_parse_batch_device_reasm (FIXED, max_layers 16): the records equal the restatement's, the info equals
    oracle_reasm over the restatement's records and pcppx_reasm_device over the engine's own."""
    import torch

    I = wc.instances()[inst]
    eng = fresh_engines(inst)
    pl = wc.placed(comp)
    g = device_parse(eng, comp, I.opts(16), reasm=True)
    osum, olay, _ = restated(comp, I.csum, 16)
    assert_records(comp, g, (osum, olay), f"{inst} fused")
    assert_equal_fields(g["info"], oracle.oracle_reasm(pl.batch, osum, olay), comp, "fused info")
    data, offsets, caplens = device_batch(comp)
    n = pl.batch.n
    st = torch.from_numpy(g["summary"].view(np.uint8).reshape(-1).copy()).to(data.device)
    lay = torch.from_numpy(np.ascontiguousarray(g["layers"]).view(np.uint8).reshape(-1).copy()).to(data.device)
    info = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device=data.device)
    eng.reasm_device(data, offsets, caplens, n, 1, st, lay, 16, info, torch.cuda.current_stream(data.device).cuda_stream)
    torch.cuda.synchronize(data.device)
    assert_equal_fields(g["info"], info.cpu().numpy().view(abi.REASM_DTYPE)[:n], comp, "fused vs pcppx_reasm_device")


@pytest.mark.gpu
@INSTANCES
def test_gpu_window_grid_lane_kernel(inst):
    """The lane-per-packet cross-check kernel (tools/ab, no LDS window at all) under each instance's options."""
    from tools import ab

    I = wc.instances()[inst]
    g = device_parse(None, "solid", I.opts(16), variant=ab.LANE)
    assert_records("solid", g, restated("solid", I.csum, 16), f"lane kernel as {inst}")


# Kinds the fast path takes nowhere on the grid, and why. Every other kind must have packets on both sides (the fast-path
# marks of tools/ab variants 30 / 31); no kind is always fast (every ladder runs past the last edge).
_NOT_L4 = "fast_walk takes only TCP, UDP or a fragment's Payload behind the last IP layer"
NEVER_FAST = {"arp": "fast_walk takes only IPv4 / IPv6 behind the VLAN tags and MPLS labels", "llc": "as arp",
              "gre1_ppp": "fast_walk takes GREv0 only", "icmp_echo": _NOT_L4, "icmp_error_ipv4": _NOT_L4}
# the 96-B window only: Ethernet + the 72-B IPv6 layer (hop-by-hop + AH) + TCP's 20 B is 106 B at the least
NEVER_FAST_96 = {"ipv6_dst_auth": "its shortest stack ends 106 B into the packet"}


def fast_shares(variant: int, csum: bool) -> tuple[float, dict[str, tuple[int, int]]]:
    """(share of the slid descriptors of the solid composition the fast path took, {kind: (fast, all)})."""
    g = device_parse(None, "solid", abi.make_opts(0, 8, csum, 16), variant=variant)
    fast = (g["summary"]["flags"] & FAST_MARK) != 0
    g["summary"] = g["summary"].copy()
    g["summary"]["flags"] &= ~np.uint16(FAST_MARK)
    assert_records("solid", g, restated("solid", csum, 16), f"tools/ab variant {variant}")  # equal up to the mark
    pl = wc.placed("solid")
    kinds = np.array([list(wc.KINDS).index(wc.grid()[u].kind) for u in pl.uid])
    per = {k: (int(fast[kinds == j].sum()), int((kinds == j).sum())) for j, k in enumerate(wc.KINDS)}
    return float(fast.mean()), per


@pytest.mark.gpu
@pytest.mark.parametrize("variant,csum", [(30, True), (31, False)], ids=["csum-96", "parse-only-96+48"])
def test_gpu_window_grid_fast_path_share(variant, csum):
    """Both walks see every header kind: some grid packet of the kind is marked fast and some is not (tools/ab variant
    30: the 96-B checksum instance; 31: a two-round 96 + 48-B parse-only instance), except the kinds listed with a
    reason (the kinds whose layers the generic walk builds -- HTTP, SSL, DNS, VXLAN, GTP -- are marked fast only where a
    cut leaves them no payload). The shares are printed: a report, not a threshold."""
    share, per = fast_shares(variant, csum)
    print(f"\nvariant {variant} (checksums {csum}): fast share of the grid {share:.4f}")
    for k, (f, n) in per.items():
        print(f"   {k:18s} fast {f:6d} of {n:6d}")
    never = sorted(k for k, (f, n) in per.items() if f == 0)
    always = sorted(k for k, (f, n) in per.items() if f == n)
    assert never == sorted({**NEVER_FAST, **(NEVER_FAST_96 if variant == 30 else {})}) and not always, (never, always)
