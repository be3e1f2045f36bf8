"""The host path's chunk staging on adversarial descriptor layouts (tests/host_cases.py).

pcppx_parse_batch_host and pcppx_filter_batch_host cut a batch into chunks, copy each either straight from the caller's
bytes or packet by packet through pinned staging, and key everything downstream to the chunk boundaries: the three reused
slots, the routing of records through the chunk's first packet, the DENSE kernels that chain their positions from chunk to
chunk on the device, the filter's sequence base and matched[] routing.

CPU (unmarked): the Python chunk-plan model carries the constants of pcppx_capi.cpp; every case produces the plan it was
built for; the plans together reach both kinds of chunk, every stop reason and both transitions; the restatement flags
exactly the descriptors a builder marked.
GPU: one reference throughout, oracle.oracle_parse over the same PacketBatch (the C restatement, pinned to the reference
project by test_oracle_*), compared bit for bit; the filter against oracle.oracle_filter (and the reference worker where it
was built).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np
import pytest

import host_cases as hc
import oracle
from pcapplusplus_amd import abi

CAPI = Path(__file__).resolve().parents[1] / "pcapplusplus_amd" / "csrc" / "pcppx_capi.cpp"

ALL = dict(hc.all_cases())
FILTER = hc.filter_cases()
BIG = {k for k, _ in hc.big_cases()}


def ids(*prefixes):
    return [k for k in ALL if k.startswith(prefixes)]


# ---------------------------------------------------------------- shared, computed once, never modified
_REF: dict = {}
_PLANS: dict = {}


def reference(key: str, case: hc.Case, csum: bool = True, ml: int | None = None):
    """The restatement's FIXED records of a case: (summary[n], layers[n, ml])."""
    ml = case.max_layers if ml is None else ml
    k = (key, csum, ml)
    if k not in _REF:
        if key in BIG:  # one big case's records at a time
            for old in [x for x in _REF if x[0] in BIG]:
                del _REF[old]
        s, lay = oracle.oracle_parse(case.batch, abi.make_opts(0, 8, csum, ml), threads=8)
        s.setflags(write=False)
        lay.setflags(write=False)
        _REF[k] = (s, lay)
    return _REF[k]


def explained(key: str):
    if key not in _PLANS:
        b = ALL[key]().batch
        _PLANS[key] = hc.explain(b.offsets, b.caplens, b.data.nbytes)
    return _PLANS[key]


def brief_of(summary):
    return summary.view(np.uint8).reshape(len(summary), 32)[:, :16].copy().view(abi.BRIEF_DTYPE).ravel()


def dense_of(summary, layers, ml):
    """The DENSE array the FIXED rows amount to: every packet's first min(n_layers, ml) entries, back to back."""
    keep = np.arange(ml)[None, :] < np.minimum(summary["n_layers"], ml)[:, None]
    return layers[keep]


# ---------------------------------------------------------------- CPU: the model and the cases
def test_model_constants():
    """The model's constants are those of pcppx_capi.cpp: retuning one there moves the cases off their edges, and fails
    here first."""
    src = CAPI.read_text()
    num = r"([0-9]+)u?(?:\s*<<\s*([0-9]+))?"

    def const(name):
        m = re.search(rf"constexpr\s+\w+\s+{name}\s*=\s*{num}\s*;", src)
        assert m, f"{name} not found in {CAPI.name}"
        return int(m.group(1)) << int(m.group(2) or 0)

    assert const("kMaxGap") == hc.K_MAX_GAP
    assert const("kMinRun") == hc.K_MIN_RUN
    assert const("kChunkBytes") == hc.K_CHUNK_BYTES
    assert const("kChunkPackets") == hc.K_CHUNK_PACKETS
    hdr = (CAPI.parents[2] / "include" / "pcppx.h").read_text()
    assert int(re.search(r"#define\s+PCPPX_MAX_CAPLEN\s+([0-9]+)", hdr).group(1)) == hc.MAX_CAPLEN == abi.MAX_CAPLEN


@pytest.mark.parametrize("key", list(ALL))
def test_case_plan(key):
    """The layout produces the plan it was built for (chunk kinds, boundaries and staged bytes)."""
    c = ALL[key]()
    got = [(x["kind"], x["i"], x["j"], x["staged"]) for x in explained(key)]
    print(key, c.name, got)
    assert got == c.plan
    assert got[0][1] == 0 and got[-1][2] == c.batch.n and all(a[2] == b[1] for a, b in zip(got, got[1:]))


def test_plans_cover_every_branch():
    """Over all cases: both kinds of chunk, every reason a direct run or a gathered chunk stops, a run declined for
    every reason a short run can stop, both transitions, and a call of at least 7 chunks."""
    direct_stops, gather_stops, declined, trans, most = set(), set(), set(), set(), 0
    for key in ALL:
        ch = explained(key)
        most = max(most, len(ch))
        for c in ch:
            (direct_stops if c["kind"] == "direct" else gather_stops).add(c["stop"])
            if c["kind"] == "gather":
                declined.add(c["run_stop"])
        trans |= {(a["kind"], b["kind"]) for a, b in zip(ch, ch[1:])}
    print(sorted(direct_stops), sorted(gather_stops), sorted(declined), sorted(trans), most)
    assert direct_stops == {hc.GAP, hc.BELOW, hc.BOUNDS, hc.BYTES, hc.PACKETS, hc.END}
    assert gather_stops == {hc.BYTES, hc.PACKETS, hc.END}
    assert declined >= {hc.GAP, hc.BELOW, hc.OVERLAP, hc.BOUNDS}
    assert trans == {("direct", "direct"), ("direct", "gather"), ("gather", "direct"), ("gather", "gather")}
    assert most >= 7


@pytest.mark.parametrize("key", list(ALL))
def test_case_inputs(key):
    """A condition on the inputs: the restatement flags exactly the descriptors the builder marked bad or oversize,
    parses nothing out of an empty one, and (outside H6, H7, H9 and the Ethernet-only H8a) at least 95% of the packets
    carry three layers or more."""
    c = ALL[key]()
    s, lay = reference(key, c)
    n = c.batch.n
    mark = lambda ix: np.isin(np.arange(n), ix)  # noqa: E731
    assert np.array_equal((s["flags"] & abi.F_BAD_DESC) != 0, mark(c.bad))
    assert np.array_equal((s["flags"] & abi.F_OVERSIZE) != 0, mark(c.oversize))
    dead = mark(c.bad) | mark(c.oversize) | mark(c.empty)
    assert np.array_equal(c.batch.caplens == 0, mark(c.empty))
    assert (s["n_layers"][dead] == 0).all() and (s["n_layers"][~dead] >= 1).all()
    assert (s["flags"][mark(c.bad)] == abi.F_BAD_DESC).all() and (s["flags"][mark(c.oversize)] == abi.F_OVERSIZE).all()
    if c.rich:
        assert not dead.any() or key == "H10"
        assert (s["n_layers"] >= 3).mean() >= 0.95
        v4 = (s["flags"] & abi.F_IP_CSUM) != 0
        assert ((s["flags"][v4] & abi.F_IP_CSUM_OK) != 0).all()  # the stamped IPv4 headers verify
    if key != "H5-same" and not key.startswith("H8a") and not key.startswith("H7"):
        live = s["hash5"][~dead]
        assert len(np.unique(live)) >= 0.49 * len(live)  # the stamp: records of different packets differ


def own_match(batch, s, lay, spec):
    """Every packet's own isMatched under spec: the worker restatement with a flow table that never remembers."""
    class Forgetful(dict):
        def __setitem__(self, k, v):
            pass

    return oracle.oracle_filter(batch, s, lay, spec, Forgetful())[0].astype(bool)


def hot_spec():
    return oracle.make_spec(src_ip=int.from_bytes(hc.HOT_ADDR, "little"))


SPECS = {"all": oracle.make_spec, "tcp": lambda: oracle.make_spec(protocol=oracle.P_TCP), "hot-src": hot_spec}


@pytest.mark.parametrize("key", ["H3", "H10"])
def test_order_sensitive_spec_reaches_the_flow_rule(key):
    """The order-sensitive spec (src_ip = the address one end of 60 flows shares): at least 100 packets match only
    because their flow matched earlier, reverse-direction packets lie both before their flow's first forward packet
    (unmatched) and after it (matched through the table), and the latter lie in more than one chunk."""
    c = dict(FILTER)[key]()
    s, lay = reference("flows-" + key, c, csum=False, ml=16)
    spec = hot_spec()
    own = own_match(c.batch, s, lay, spec)
    m = oracle.oracle_filter(c.batch, s, lay, spec)[0].astype(bool)
    by_flow = m & ~own
    hot = np.isin(s["hash5"], np.unique(s["hash5"][own]))
    early = hot & ~m
    print(key, "own", int(own.sum()), "through the flow rule", int(by_flow.sum()), "before the first forward",
          int(early.sum()))
    assert by_flow.sum() >= 100 and early.sum() >= 10 and not (m & ~hot).any()
    chunks = hc.plan(c.batch.offsets, c.batch.caplens, c.batch.data.nbytes)
    assert chunks == c.plan and len(chunks) >= 2
    assert sum(1 for _, i, j, _ in chunks if by_flow[i:j].any() and own[i:j].any()) >= 2


# ---------------------------------------------------------------- GPU: parse
def check_fixed(got, want):
    oracle.compare_exact(got[0], got[1], want[0], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(ALL))
def test_gpu_fixed_records(engine, key):
    """Summary and FIXED layer rows, checksums on, pageable input and output."""
    c = ALL[key]()
    want = reference(key, c)
    got = engine.parse_host(c.batch, abi.make_opts(0, 8, True, c.max_layers))
    check_fixed(got, want)
    dead = abi.F_BAD_DESC | abi.F_OVERSIZE
    assert np.array_equal(got[0]["flags"] & dead, want[0]["flags"] & dead)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(ALL))
def test_gpu_deep_window(engine, key):
    """The same records through the two-round window (PCPPX_WINDOW_DEEP)."""
    c = ALL[key]()
    got = engine.parse_host(c.batch, abi.make_opts(0, 8, True, c.max_layers, abi.WINDOW_DEEP))
    check_fixed(got, reference(key, c))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ids("H3", "H4", "H10"))
def test_gpu_parse_only_short_window(engine, key):
    """Parse-only launches through the one-round window (PCPPX_WINDOW_SHORT)."""
    c = ALL[key]()
    got = engine.parse_host(c.batch, abi.make_opts(0, 8, False, c.max_layers, abi.WINDOW_SHORT))
    check_fixed(got, reference(key, c, csum=False))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ids("H2", "H3", "H4", "H6", "H10"))
def test_gpu_pinned_in_and_out(engine, key):
    """Page-locked input and page-locked record arrays: each chunk's records are written by DMA at the chunk's first
    packet in the caller's arrays (no drain copy)."""
    from pcapplusplus_amd.engine import pinned_copy, pinned_records

    c = ALL[key]()
    pb, buf = pinned_copy(c.batch)
    out, keep = pinned_records(c.batch.n, c.max_layers)
    try:
        out[0].view(np.uint8)[:] = 0xA5  # a record nobody writes cannot pass for one
        out[1].view(np.uint8)[:] = 0xA5
        s, lay = engine.parse_host(pb, abi.make_opts(0, 8, True, c.max_layers), out)
        got = (s.copy(), lay.copy())
    finally:
        del out
        for k in keep:
            k.free()
        buf.free()
    check_fixed(got, reference(key, c))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ids("H3", "H6", "H10"))
def test_gpu_brief_only(engine, key):
    """No summary: the 16-B brief and the FIXED rows."""
    c = ALL[key]()
    want = reference(key, c)
    _, br, lay, w = engine.parse_host_ex(c.batch, abi.make_opts(0, 8, True, c.max_layers), want_summary=False,
                                         want_brief=True)
    assert br.tobytes() == brief_of(want[0]).tobytes()
    assert w == c.batch.n * c.max_layers
    oracle.compare_exact(want[0], lay.reshape(c.batch.n, c.max_layers), want[0], want[1])


def check_dense(engine, case, want, ml, src, pinned):
    o = abi.make_opts(0, 8, True, ml, layout=abi.LAYOUT_DENSE)
    s, br, dense, w = engine.parse_host_ex(case.batch, o, want_summary=src == "summary", want_brief=src == "brief",
                                           pinned=pinned)
    exp = dense_of(want[0], want[1], ml)
    assert w == len(exp) == len(dense), (w, len(exp), len(dense))
    assert dense.tobytes() == exp.tobytes()
    if s is not None:
        assert s.tobytes() == want[0].tobytes()
    else:
        assert br.tobytes() == brief_of(want[0]).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("src", ["brief", "summary"])
@pytest.mark.parametrize("key", ids("H2-run4095", "H2-run4096", "H3", "H5", "H6", "H7", "H8a", "H10"))
def test_gpu_dense_layout(engine, key, src, pinned):
    """PCPPX_LAYOUT_DENSE: the chains back to back, their positions chained on the device from chunk to chunk (eight
    chunks in H3: every slot's cumulative count is read by a successor), with chains of length 0 (bad, oversize and empty
    packets) at the start and the end of a 1024-packet block and of a chunk; lengths from the brief or the summary; into
    the slot's staging or straight into a page-locked caller array. layers_written is the array's length."""
    c = ALL[key]()
    check_dense(engine, c, reference(key, c), c.max_layers, src, pinned)


@pytest.mark.gpu
@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("ml", [1, 16])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
def test_gpu_dense_block_edges(engine, n, ml, pinned):
    """DENSE at the edges of the compaction's 1024-packet block, with max_layers 1 and 16."""
    c = hc.h1_slice(n)
    assert hc.plan(c.batch.offsets, c.batch.caplens, c.batch.data.nbytes) == c.plan
    want = oracle.oracle_parse(c.batch, abi.make_opts(0, 8, True, ml))
    for src in ("brief", "summary"):
        check_dense(engine, c, want, ml, src, pinned)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ids("H3", "H6", "H10"))
def test_gpu_flow_key_column(engine, key):
    """pcppx_records.flow_keys on the host path: every packet's hash5, routed chunk by chunk."""
    import ctypes as C

    c = ALL[key]()
    want = reference(key, c)
    n = c.batch.n
    for with_summary in (True, False):
        s = np.zeros(n, dtype=abi.SUMMARY_DTYPE)
        br = np.zeros(n, dtype=abi.BRIEF_DTYPE)
        fk = np.full(n, 0xA5A5A5A5, dtype=np.uint32)
        rec = abi.Records(s.ctypes.data if with_summary else None, None, fk.ctypes.data)
        rec.brief = None if with_summary else br.ctypes.data
        b = c.batch.c_batch()
        o = abi.make_opts(0, 8, True, 0)
        abi.check(engine.lib.pcppx_parse_batch_host(engine.ctx, C.byref(b), C.byref(o), C.byref(rec)), "host")
        assert np.array_equal(fk, want[0]["hash5"])


@pytest.mark.gpu
def test_gpu_two_calls_on_one_context(engine):
    """H10 (two chunks, DENSE) and then H3 (eight chunks) on the same context: the second call starts from idle slots
    and carries over no chunk, count or position of the first."""
    a, b = ALL["H10"](), ALL["H3"]()
    wa, wb = reference("H10", a), reference("H3", b)
    for pinned in (False, True):
        check_dense(engine, a, wa, a.max_layers, "brief", pinned)
        check_dense(engine, b, wb, b.max_layers, "brief", pinned)
        check_fixed(engine.parse_host(b.batch, abi.make_opts(0, 8, True, b.max_layers)), wb)
        check_fixed(engine.parse_host(a.batch, abi.make_opts(0, 8, True, a.max_layers)), wa)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["H9-run", "H9-gathered", "H9-huge"])
def test_gpu_oversize_flag(engine, key):
    """An in-bounds packet above PCPPX_MAX_CAPLEN is PCPPX_F_OVERSIZE on the host path as on the device path, in a
    direct chunk and in a gathered one, below and above the 64 MiB a chunk stages (it stages no bytes)."""
    c = ALL[key]()
    s, _ = engine.parse_host(c.batch, abi.make_opts(0, 8, True, c.max_layers))
    print(key, [hex(int(x)) for x in s["flags"][c.oversize]])
    assert (s["flags"][c.oversize] == abi.F_OVERSIZE).all()
    assert ((s["flags"] & (abi.F_OVERSIZE | abi.F_BAD_DESC)) != 0).sum() == len(c.oversize)


# ---------------------------------------------------------------- GPU: filter
def filter_reference(key, case):
    return reference("flows-" + key, case, csum=False, ml=16)


@pytest.mark.gpu
@pytest.mark.parametrize("spec_name", list(SPECS))
@pytest.mark.parametrize("k", range(len(FILTER)), ids=[x for x, _ in FILTER])
def test_gpu_filter_host(engine, k, spec_name):
    """pcppx_filter_batch_host over a case and then, on the same context, over the next one: matched[] and every
    counter equal the worker restatement's, the flow table and the sequence numbers carried across chunks and calls."""
    spec = SPECS[spec_name]()
    (key, mk), (key2, mk2) = FILTER[k], FILTER[(k + 1) % len(FILTER)]
    c, c2 = mk(), mk2()
    assert c.batch.n <= 33_000 and c2.batch.n <= 33_000
    s, lay = filter_reference(key, c)
    s2, lay2 = filter_reference(key2, c2)
    engine.filter_reset(1 << 12)
    gm, gst = engine.filter_host(c.batch, spec)
    table: dict = {}
    om, ost = oracle.oracle_filter(c.batch, s, lay, spec, table)
    bad = np.nonzero(gm != om)[0]
    assert len(bad) == 0, (key, spec_name, len(bad), bad[:10])
    for f in abi.STATS_FIELDS:
        assert gst[f] == ost[f], (key, f, gst[f], ost[f])
    assert ost["needs_host_count"] == len(c.bad) and ost["flow_table_full"] == 0
    if oracle.ref_available() and len(c.bad) == 0:
        rm, rst = oracle.ref_filter(c.batch, spec)
        assert np.array_equal(gm, rm)
        for f in abi.STATS_FIELDS:
            if f != "needs_host_count":
                assert gst[f] == rst[f], (key, f, gst[f], rst[f])
    gm2, gst2 = engine.filter_host(c2.batch, spec)
    om2, ost2 = oracle.oracle_filter(c2.batch, s2, lay2, spec, table)
    bad = np.nonzero(gm2 != om2)[0]
    assert len(bad) == 0, (key2, spec_name, len(bad), bad[:10])
    for f in abi.STATS_FIELDS:
        assert gst2[f] == ost[f] + ost2[f], (key2, f, gst2[f], ost[f] + ost2[f])
