"""Packets, spans and outputs on both sides of 2^32 (layouts: tests/wide_cases.py).

Every kernel takes 64-bit packet offsets and forms addresses as data + offset. Two lines cut a batch of 4 GiB and more:
the offset line (packet offset 2^32) and the address line (the data offset whose device address is a multiple of 2^32).
A value kept in 32 bits at either one is silent: wrong checksums, wrong copied bytes, a wrong overflow verdict.

CPU: the layout function puts both lines where the packets are for any base pointer; the stages hold every packet
edge, straddle, packet type, tile form and bad descriptor they are meant to, at both lines; the restatement of the
compact batches equals the plain-Python RFC 1071 values; the period's byte sums are odd, and R repetitions of it give
R shifted copies of one period's output (pcppx_select_reference / pcppx_steer_reference).
GPU: over a 4 GiB + 128 MiB source of which only the extents are ever written, every byte-reading kernel -- the
checksum parse, the parse-only instances, the lane kernel, the reassembly front ends, the filter, select and steer --
is bit-exact against the restatement of the same packets in a small buffer; the host path over an mmap of the same
size likewise; and select / steer outputs of 4.25 GiB (a 1 MiB source, one period of 251 descriptors repeated) hold
exactly the shifted copies, with the capacity verdicts exact at 2^32 - 1.
"""
from __future__ import annotations

import mmap
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest

import checksum_cases as cc
import oracle
import select_cases as sc
import steer_cases as tc
import wide_cases as wc
from pcapplusplus_amd import abi
from pcapplusplus_amd.pcap import PacketBatch
from test_checksums import check_against_python
from test_filter import OPTS as FILTER_OPTS
from test_filter import compare_stats, specs_for
from test_reasm import assert_equal_info
from test_reasm import restated as reasm_restated

DEV = "cuda:0"
LINE, MIB = wc.LINE, wc.MIB
M32 = LINE - 1
MIS = (0, 5)
# hypothetical allocation addresses: 4 GiB-aligned, just below and just above a multiple of 4 GiB, in the middle, and ones
# that put the first address line next to either end of the margin
BASES = (0x7F00_0000_0000, 0x7F01_0000_0000 - 4096, 0x7F01_0000_0000 - 2 * MIB, 0x7F00_0000_0000 + 4096,
         0x7F00_8000_0000 + 512, 0x7F01_0000_0000 - 16 * MIB - 64, 0x7F01_0000_0000 - 16 * MIB - 65,
         0x7F00_0000_0000 + 16 * MIB, 0x7F00_0000_0000 + 16 * MIB - 512, 0x7EFF_E000_0200)
CSUM_OPTS = [(w, lo) for w in (abi.WINDOW_DEFAULT, abi.WINDOW_DEEP) for lo in (abi.LAYOUT_FIXED, abi.LAYOUT_PACKED)]
PARSE_ONLY = [(w, ml) for w in (abi.WINDOW_DEFAULT, abi.WINDOW_SHORT) for ml in (12, 0)]


# ---------------------------------------------------------------- CPU: the layouts
@pytest.mark.parametrize("mis", MIS)
@pytest.mark.parametrize("base", BASES, ids=hex)
def test_layout_puts_both_lines_among_the_packets(base, mis):
    lay = wc.layout(base, mis)  # (asserts its own conditions)
    data_ptr = base + lay.pad
    assert data_ptr % 16 == mis
    oA = (-data_ptr) % LINE
    assert lay.addr_line in (oA, oA + LINE) and (data_ptr + lay.addr_line) % LINE == 0
    assert 16 * MIB <= lay.addr_line and abs(lay.addr_line - LINE) >= 16 * MIB
    assert lay.data_len > LINE + 32 * MIB and lay.addr_line + 16 * MIB <= lay.data_len
    assert lay.pad >= 64 and lay.pad + lay.data_len + 64 <= wc.RAW_BYTES


@pytest.fixture(scope="module")
def cpu_stages():
    return {b: (wc.layout(b, 5), wc.stages(wc.layout(b, 5))) for b in (BASES[0], BASES[1])}


def _l4_hdr(p: cc.Pkt) -> int:
    return 20 if p.family.endswith("TCP") else 8


@pytest.mark.parametrize("base", BASES[:2], ids=hex)
def test_stages_cover_both_lines(cpu_stages, base):
    """Every item the wide batch is there for, from the generated layout, at the offset line and at the address line."""
    lay, stages = cpu_stages[base]
    dl = lay.data_len
    by = {s.name: s for s in stages}
    for s in stages:  # whole tiles per line, inside the data with slack, and the stream criterion on the side meant
        assert s.n % 64 == 0
        for t in range(s.n // 64):
            assert len({d.line for d in s.descs[64 * t:64 * t + 64]}) == 1, s.name
        assert all(o >= 64 and o + len(a) <= dl for o, a in s.extents), s.name
        assert sum(len(a) for _, a in s.extents) < MIB, s.name
        want = {"sparse": False, "bad_desc": False}.get(s.name, True)  # bad_desc: one packet at the far end of the data
        assert s.stream == [want] * (s.n // 64), (s.name, s.stream)
    for li, L in enumerate(lay.lines):
        ds = [(s, d) for s in stages for d in s.descs if d.line == li]
        live = [d for _, d in ds if not d.dead]
        # packet edges on the line
        assert any(d.off == L and d.cap > 0 for d in live)
        assert any(d.off + d.cap == L and d.cap > 0 for d in live)
        assert any(d.off == L and d.cap == 0 and d.dead == cc.DEAD_EMPTY for _, d in ds)
        assert any(d.off == L + 1 for d in live) and any(d.off == L - 1 for d in live)
        assert any(d.off + d.cap == L + 1 for d in live)
        # straddles
        strad = [d for d in live if d.k is not None]
        assert all(d.off < L < d.off + d.cap and L - d.off == d.k for d in strad) and len(strad) >= 60
        assert not any(wc.straddles(d, L) for d in live if d.k is None)

        def tagged(prefix):
            got = [d for d in strad if d.tag.startswith(prefix)]
            assert got, prefix
            return got

        assert all(0 < d.k < 14 for d in tagged("eth"))
        for d in tagged("ip_addr"):
            lo, hi = (14 + 12, 14 + 20) if d.pkt.family.startswith("IPv4") else (14 + 8, 14 + 40)
            assert lo < d.k < hi and d.pkt.l4_off == hi
        assert {d.pkt.family for d in tagged("ip_addr")} == set(cc.FAMILIES)
        assert all(d.pkt.l4_off < d.k < d.pkt.l4_off + 4 for d in tagged("l4_ports"))
        for d in tagged("l4_csum"):  # the line between the two bytes of the stored checksum
            at = d.pkt.l4_off + (16 if d.pkt.family.endswith("TCP") else 6)
            assert d.k == at + 1
        for pre in ("l4_ports", "l4_csum", "l4_edge/", "l4_edge5", "l4_whole", "l4_tail"):
            assert {d.pkt.family for d in tagged(pre)} == set(cc.FAMILIES), pre
        assert all(d.pkt.l4_off < d.k < d.pkt.l4_off + 16 for d in tagged("l4_edge5"))
        assert all(d.pkt.l4_off + _l4_hdr(d.pkt) < d.k < d.pkt.l4_off + _l4_hdr(d.pkt) + 16 for d in tagged("l4_edge/"))
        assert all(d.pkt.l4_off + 32 <= d.k <= d.cap - 32 for d in tagged("l4_whole"))
        assert all(d.cap - 16 < d.k < d.cap for d in tagged("l4_tail"))
        gaps = {d.k for d in tagged("window_gap")}
        assert gaps >= {96, 128, 144} and any(96 < k < 128 for k in gaps) and any(128 < k < 144 for k in gaps)
        assert all(d.cap > 160 for d in tagged("window_gap"))
        for pre in ("deep", "http"):  # beyond both windows: the generic walk and the hashes read these from HBM
            assert all(d.pkt is None and 144 < d.k < d.cap - 16 for d in tagged(pre)) and len(tagged(pre)) >= 3
        assert all(14 < d.k < 22 or d.k > 62 for d in tagged("vlan")) and len(tagged("vlan")) == 2
        assert len(tagged("gre")) == 2
        # packet types and verdicts among the straddlers
        known = [d.pkt for d in strad if d.pkt is not None]
        assert {p.family for p in known} == set(cc.FAMILIES)
        assert any(p.l4_calc != p.l4_stored for p in known) and any(p.l4_calc == p.l4_stored for p in known)
        assert any(p.has_ip4 and p.ip_calc != p.ip_stored for p in known)
        # tile forms
        perm = [d for d in by["permuted"].descs if d.line == li]
        first, rest = perm[0], perm[1:]
        assert first.off > L and all(d.off + d.cap <= first.off for d in rest) and any(wc.straddles(d, L) for d in rest)
        sp = [d for d in by["sparse"].descs if d.line == li]
        assert min(d.off for d in sp) < L - 6 * MIB and max(d.off for d in sp) > L + 6 * MIB
        assert sum(1 for a, b in zip(sp, sp[1:]) if b.off - a.off > MIB) >= 12 and any(wc.straddles(d, L) for d in sp)
        dd = [d for d in by["dead"].descs if d.line == li]
        assert {d.dead for d in dd} == {0, cc.DEAD_BAD_DESC, cc.DEAD_EMPTY} and any(wc.straddles(d, L) for d in dd)
        assert any(d.dead == cc.DEAD_EMPTY and abs(d.off - L) < 8192 for d in dd)
        big = [d for d in by["tile1500"].descs if d.line == li]
        assert [d.dead for d in big] == [cc.DEAD_OVERSIZE] + [0] * 63 and big[0].cap == 65536 and wc.straddles(big[0], L)
        big = big[1:]
        assert all(d.cap == 1500 for d in big) and any(wc.straddles(d, L) for d in big)
        smin, emax = min(d.off for d in big), max(d.off + d.cap for d in big)
        assert emax - smin > 40 * 2048 and smin + 20 * 2048 < L < emax - 20 * 2048  # 2 KiB stream windows
    # bad descriptors against a data_len above 2^32
    bad = {d.tag: d for d in by["bad_desc"].descs}
    assert dl > LINE
    d = bad["ends_at_data_len"]
    assert d.off + d.cap == dl and not d.dead and d.off > LINE
    assert (d.off & M32) + d.cap <= (dl & M32) < LINE  # in bounds although its low dword plus the caplen is far from 2^32
    d = bad["ends_1_past_data_len"]
    assert d.off + d.cap == dl + 1 and d.dead == cc.DEAD_BAD_DESC
    for tag in ("in_bounds_in_32_bits", "in_bounds_in_32_bits_b"):
        d = bad[tag]
        assert d.off > dl and (d.off & M32) + d.cap <= dl and d.dead == cc.DEAD_BAD_DESC, tag
    assert (bad["in_bounds_in_32_bits"].off & M32) + 64 <= (dl & M32)  # ... and against a truncated data_len as well
    d = bad["wraps_64_bits"]
    assert d.off == 0xFFFFFFFFFFFFFFF0 and (d.off + d.cap) >> 64 and ((d.off + d.cap) & (2**64 - 1)) <= dl
    assert bad["at_data_len"].off == dl and bad["at_data_len"].cap == 1 and bad["empty_at_data_len"].cap == 0
    n_bad = sum(1 for d in by["bad_desc"].descs if d.dead == cc.DEAD_BAD_DESC)
    assert n_bad == 10 and all((not wc.in_bounds(d.off, d.cap, dl)) == (d.dead == cc.DEAD_BAD_DESC)
                               for s in stages for d in s.descs)


@pytest.mark.parametrize("base", BASES[:2], ids=hex)
def test_compact_restatement_equals_python_reference(cpu_stages, base):
    """The compact batches the expected records come from: the restatement's checksum fields and verdict bits equal the
    plain-Python RFC 1071 values on every packet checksum_cases built, at the alignments of the wide layout; and the
    compact batch holds the bytes of the extents. The dead rows pin the restatement's bounds rule too: every descriptor
    that is out of bounds is PCPPX_F_BAD_DESC and nothing else, among them `wraps_64_bits`, whose end wraps 64 bits
    (the restatement once took it as in bounds and parsed the 16 bytes in front of the buffer)."""
    _, stages = cpu_stages[base]
    total = wraps = 0
    for st in stages:
        s, lay = oracle.oracle_parse(st.compact, abi.make_opts(0, 8, True, 12))
        idx = st.known()
        check_against_python(st.case_batch(), s[idx], f"restatement {st.name}")
        total += len(idx)
        for i, d in enumerate(st.descs):
            if d.tag == "wraps_64_bits":
                assert int(st.compact.offsets[i]) == 0xFFFFFFFFFFFFFFF0 and int(st.compact.caplens[i]) == 64
                assert int(s["flags"][i]) == abi.F_BAD_DESC and int(s["n_layers"][i]) == 0
                wraps += 1
    assert total > 8000 and wraps == 2


@pytest.mark.parametrize("K", [0, 3, 64])
def test_period_sums_are_odd_and_repetitions_are_shifted_copies(K):
    """The period of part 3: odd byte sums (every repetition on a new destination alignment), enough repetitions to pass
    2^32 + 2^28 with more than three 256-block scan steps, and -- on three repetitions, through the reference -- the
    output of R periods is R shifted copies of one period's output."""
    p = wc.period(K)
    sums = p.sums()
    assert all(s % 2 == 1 for s in sums), sums
    S = sum(sums)
    R = wc.repeats(S)
    assert R * S >= LINE + (1 << 28) and (R - 1) * S < LINE + (1 << 28) and R * wc.P > 3 * 256 * 1024
    assert wc.P == 251 and (p.caplens[40:47] == 0).all() and {9000, 65535} <= set(p.caplens.tolist())
    assert int((p.offsets + p.caplens).max()) <= len(p.block) == MIB
    if K == 0:
        assert 0.65 < (p.keep != 0).mean() < 0.85
    else:
        assert (p.bucket >= K).sum() >= 5 and {int(b) for b in p.bucket if b < K} == set(range(K))
        # K = 3: bucket 1 alone holds more than 2^32 bytes (steer's block byte prefix is relative to the bucket), and
        # bucket_pos[2] and [3] are >= 2^32
        assert K != 3 or (R * sums[1] >= LINE + (1 << 26) and R * (sums[0] + sums[1]) >= LINE and min(sums) > 0)
    one, three = period_reference(p, 1), period_reference(p, 3)
    exp = expected_repeats(p, one, 3)
    for f, want in exp.items():
        got = getattr(three, f)
        assert np.array_equal(got[:len(want)], want), f
    assert three.data[:3 * S].tobytes() == expected_bytes(p, one, 3).tobytes()


def period_case(p: wc.Period, R: int, **kw):
    offs, caps = np.tile(p.offsets, R), np.tile(p.caplens, R)
    if p.keep is not None:
        return sc.Case(f"period x{R}", p.block, offs, caps, keep=np.tile(p.keep, R), **kw)
    return tc.Case(f"period k{p.K} x{R}", p.block, offs, caps, n_buckets=p.K, bucket=np.tile(p.bucket, R), **kw)


def period_reference(p: wc.Period, R: int, **kw):
    c = period_case(p, R, **kw)
    return sc.run_reference(c) if p.keep is not None else tc.run_reference(c)


def period_groups(p: wc.Period, one) -> list[tuple[int, int, int, int]]:
    """Per output group (select: one; steer: each bucket) of one period: (first rank, packets, first byte, bytes)."""
    if p.keep is not None:
        return [(0, int(one.totals[abi.SEL_WRITTEN_PACKETS]), 0, int(one.totals[abi.SEL_WRITTEN_BYTES]))]
    f, q = one.bucket_first.astype(np.int64), one.bucket_pos.astype(np.int64)
    return [(int(f[b]), int(f[b + 1] - f[b]), int(q[b]), int(q[b + 1] - q[b])) for b in range(p.K)]


def expected_repeats(p: wc.Period, one, R: int) -> dict:
    """offsets / caplens / index (and bucket_first / bucket_pos) of R repetitions, from one period's reference output."""
    offs, caps, idx = [], [], []
    r = np.arange(R, dtype=np.int64)[:, None]
    pos = 0
    for first, cnt, at, nbytes in period_groups(p, one):
        sl = slice(first, first + cnt)
        offs.append((pos + (one.offsets[sl].astype(np.int64) - at)[None, :] + r * nbytes).reshape(-1))
        caps.append(np.tile(one.caplens[sl], R))
        idx.append((one.index[sl].astype(np.int64)[None, :] + r * wc.P).reshape(-1))
        pos += R * nbytes
    out = {"offsets": np.concatenate(offs).astype(np.uint64), "caplens": np.concatenate(caps),
           "index": np.concatenate(idx).astype(np.uint32)}
    if p.keep is None:
        out["bucket_first"] = (one.bucket_first[:p.K + 1].astype(np.int64) * R).astype(np.uint32)
        out["bucket_pos"] = (one.bucket_pos[:p.K + 1].astype(np.int64) * R).astype(np.uint64)
    return out


def expected_bytes(p: wc.Period, one, R: int) -> np.ndarray:
    return np.concatenate([np.tile(one.data[at:at + nb], R) for _, _, at, nb in period_groups(p, one)])


# ---------------------------------------------------------------- GPU: the wide source
_wide: dict[int, SimpleNamespace] = {}


def drop_wide() -> None:
    """Release the wide source: the handle's tensors are deleted (whoever still holds the handle holds no memory), and
    the allocator's cache is emptied."""
    if _wide:
        import torch

        for w in _wide.values():
            del w.raw, w.data
        _wide.clear()
        torch.cuda.empty_cache()


def assert_no_wide_source(what: str) -> None:
    """One wide allocation at a time: before `what` allocates its own, nothing of that size is alive on the device."""
    import torch

    drop_wide()
    torch.cuda.empty_cache()
    alive = torch.cuda.memory_allocated(DEV)
    assert alive < 1 << 30, f"{what}: {alive} bytes of tensors are still alive on the device"


def get_wide(mis: int) -> SimpleNamespace:
    """The wide source with data.data_ptr() % 16 == mis: one alive at a time, never filled as a whole."""
    import torch

    if mis not in _wide:
        drop_wide()
        try:
            raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device=DEV)
        except Exception as e:  # no skip for "too big"
            pytest.fail(f"cannot allocate the wide source of {wc.RAW_BYTES} bytes (2^32 + 2^27): {e}")
        lay = wc.layout(raw.data_ptr(), mis)
        data = raw[lay.pad: lay.pad + lay.data_len]
        oA = (-data.data_ptr()) % LINE
        assert data.data_ptr() % 16 == mis
        assert lay.addr_line in (oA, oA + LINE) and lay.addr_line >= 16 * MIB and abs(lay.addr_line - LINE) >= 16 * MIB
        assert data.numel() == lay.data_len > LINE + 32 * MIB
        _wide[mis] = SimpleNamespace(raw=raw, data=data, lay=lay, stages=wc.stages(lay), restated={})
    return _wide[mis]


@pytest.fixture(scope="module", params=MIS, ids=lambda m: f"mis{m}")
def wide_mis(request):
    """The misalignment of the wide source only: pytest caches a module-scoped value until the module ends, so the
    tensors stay out of it. Each test takes the source with get_wide(wide_mis), and drop_wide() really frees it."""
    yield request.param
    drop_wide()


def put(w, st):
    """Upload a stage's extents into the wide buffer; its descriptors as device tensors."""
    import torch

    for off, a in st.extents:
        w.data[off:off + len(a)] = torch.from_numpy(a).to(DEV)
    return (torch.from_numpy(st.offsets.view(np.int64)).to(DEV), torch.from_numpy(st.caplens.view(np.int32)).to(DEV))


def restated(w, st, opts):
    # the window and the layout are not in the key: they choose a kernel instance and the device's layer packing, and
    # the restatement has neither (it takes no notice of opts.window / opts.layout)
    key = (st.name, opts.want_checksums, opts.max_layers)
    if key not in w.restated:
        w.restated[key] = oracle.oracle_parse_tuples(st.compact, abi.make_opts(0, 8, bool(opts.want_checksums),
                                                                               opts.max_layers))
    return w.restated[key]


def device_records(engine, data, offs, caps, n, opts, lane=False, summary=True, brief=False, tuples=False,
                   flow_keys=False) -> dict:
    """engine.parse_on_device_ex over tensors that are on the device already (lane: the tools' lane kernel)."""
    import torch

    ml = opts.max_layers
    z = lambda k, dt=torch.uint8: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    st = z(n * 32) if summary else None
    lay = z(max(n * ml, 1) * 8)
    tp = z(n * 48) if tuples else None
    fk = z(n, torch.int32) if flow_keys else None
    br = z(n * 16) if brief else None
    stream = torch.cuda.current_stream(DEV).cuda_stream
    if lane:
        from tools import ab

        ab.parse_device(data, offs, caps, n, 1, opts, st, lay if ml else None, stream, ab.LANE)
    else:
        engine.parse_device(data, offs, caps, n, 1, opts, st, lay if ml else None, stream, flow_keys=fk, tuples=tp,
                            brief=br)
    torch.cuda.synchronize(DEV)
    out = {}
    if st is not None:
        out["summary"] = st.cpu().numpy().view(abi.SUMMARY_DTYPE)[:n]
    if br is not None:
        out["brief"] = br.cpu().numpy().view(abi.BRIEF_DTYPE)[:n]
    raw = lay.cpu().numpy().view(abi.LAYER_DTYPE)[: n * ml]
    if ml and opts.layout == abi.LAYOUT_PACKED:
        out["layers"] = abi.unpack_layers(out["summary"] if st is not None else out["brief"], raw, ml)
    else:
        out["layers"] = raw.reshape(n, ml)
    if tp is not None:
        out["tuples"] = tp.cpu().numpy().view(abi.TUPLE_DTYPE)[:n]
    if fk is not None:
        out["flow_keys"] = fk.cpu().numpy().view(np.uint32)[:n]
    return out


def brief_of(summary: np.ndarray) -> np.ndarray:
    return summary.view(np.uint8).reshape(len(summary), 32)[:, :16].copy().view(abi.BRIEF_DTYPE).ravel()


def compare_layers(g, s, lay, ml, what):
    """FIXED entries, or PACKED ones decoded: equal inside every chain (PACKED leaves nothing past a chain)."""
    if not ml:
        return
    valid = np.arange(ml)[None, :] < np.minimum(s["n_layers"], ml)[:, None]
    zero = np.zeros(1, abi.LAYER_DTYPE)
    assert np.where(valid, g, zero).tobytes() == np.where(valid, lay, zero).tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("window,layout", CSUM_OPTS, ids=["default-fixed", "default-packed", "deep-fixed", "deep-packed"])
def test_gpu_wide_checksum_parse(engine, wide_mis, window, layout):
    """The checksum instances (span stream, whole-chunk sums from HBM, edge chunks, header windows) over every stage:
    bit-exact against the restatement of the compact batch, and against the plain-Python RFC 1071 values."""
    wide = get_wide(wide_mis)
    opts = abi.make_opts(0, 8, True, 12, window, layout)
    for st in wide.stages:
        offs, caps = put(wide, st)
        g = device_records(engine, wide.data, offs, caps, st.n, opts)
        s, lay, _ = restated(wide, st, opts)
        try:
            oracle.compare_exact(g["summary"], lay if layout == abi.LAYOUT_PACKED else g["layers"], s, lay)
            compare_layers(g["layers"], s, lay, 12, st.name)
            idx = st.known()
            check_against_python(st.case_batch(), g["summary"][idx], f"device {st.name}")
        except AssertionError as e:
            raise AssertionError(f"stage {st.name} (lines {[hex(x) for x in wide.lay.lines]}): {e}") from None


@pytest.mark.gpu
@pytest.mark.parametrize("window,ml", PARSE_ONLY, ids=["default-ml12", "default-ml0", "short-ml12", "short-ml0"])
def test_gpu_wide_parse_only(engine, wide_mis, window, ml):
    """The parse-only instances with every output (summary, brief, tuples, the flow_keys column), and without the
    summary."""
    wide = get_wide(wide_mis)
    opts = abi.make_opts(0, 8, False, ml, window)
    for st in wide.stages:
        offs, caps = put(wide, st)
        s, lay, tup = restated(wide, st, opts)
        g = device_records(engine, wide.data, offs, caps, st.n, opts, brief=True, tuples=True, flow_keys=True)
        h = device_records(engine, wide.data, offs, caps, st.n, opts, summary=False, brief=True, tuples=True)
        try:
            oracle.compare_exact(g["summary"], g["layers"], s, lay)
            assert g["brief"].tobytes() == brief_of(s).tobytes() == h["brief"].tobytes()
            assert g["tuples"].tobytes() == tup[:st.n].tobytes() == h["tuples"].tobytes()
            assert np.array_equal(g["flow_keys"], s["hash5"])
            compare_layers(h["layers"], s, lay, ml, st.name)
        except AssertionError as e:
            raise AssertionError(f"stage {st.name} (lines {[hex(x) for x in wide.lay.lines]}): {e}") from None


@pytest.mark.gpu
def test_gpu_wide_lane_kernel(engine, wide_mis):
    """The lane-per-packet cross-check kernel (it streams whole packets from HBM) under the same options."""
    wide = get_wide(wide_mis)
    for csum, ml, window in ((True, 12, abi.WINDOW_DEFAULT), (True, 12, abi.WINDOW_DEEP), (False, 12, abi.WINDOW_DEFAULT),
                             (False, 0, abi.WINDOW_SHORT)):
        opts = abi.make_opts(0, 8, csum, ml, window)
        for st in wide.stages:
            offs, caps = put(wide, st)
            g = device_records(engine, wide.data, offs, caps, st.n, opts, lane=True)
            s, lay, _ = restated(wide, st, opts)
            try:
                oracle.compare_exact(g["summary"], g["layers"], s, lay)
                if csum:
                    check_against_python(st.case_batch(), g["summary"][st.known()], f"lane {st.name}")
            except AssertionError as e:
                raise AssertionError(f"stage {st.name} (lines {[hex(x) for x in wide.lay.lines]}): {e}") from None


SEQ_BASE = 1000  # the filter's sequence number of a batch's first packet


def _filter_run(engine, data, offs, caps, n, spec):
    import torch

    ml = FILTER_OPTS.max_layers
    cap = 1 << 12
    z = lambda k, dt=torch.uint8: torch.zeros(k, dtype=dt, device=DEV)  # noqa: E731
    summary, layers, matched = z(n * 32), z(n * ml * 8), z(n)
    keys, first, stats = z(cap, torch.int64), z(cap, torch.int64), z(len(abi.STATS_FIELDS), torch.int64)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    engine.parse_device(data, offs, caps, n, 1, FILTER_OPTS, summary, layers, stream)
    engine.filter_device(data, offs, caps, n, 1, summary, layers, ml, spec, SEQ_BASE, keys, first, cap, matched,
                         stats, stream)
    torch.cuda.synchronize(DEV)
    k = keys.cpu().numpy().view(np.uint64)
    table = dict(zip(k[k != 0].tolist(), first.cpu().numpy()[k != 0].tolist()))
    return matched.cpu().numpy(), table, stats.cpu().numpy().tolist()


@pytest.mark.gpu
def test_gpu_wide_reasm_and_filter(engine, wide_mis):
    """The reassembly front ends (separate and fused with the parse) against the restatement, and the filter -- matched[],
    the flow table and the counters -- against its own run over the compact batch (every packet) and against the
    restatement's worker (the packets the device settles, in every stage)."""
    wide = get_wide(wide_mis)
    import torch

    from pcapplusplus_amd.engine import to_device

    ml = 16
    opts = abi.make_opts(0, 8, False, ml)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    matched_total = 0
    for st in wide.stages:
        offs, caps = put(wide, st)
        n = st.n
        want = reasm_restated(st.compact, opts)
        summary = torch.zeros(n * 32, dtype=torch.uint8, device=DEV)
        layers = torch.zeros(n * ml * 8, dtype=torch.uint8, device=DEV)
        info = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device=DEV)
        engine.parse_device(wide.data, offs, caps, n, 1, opts, summary, layers, stream)
        engine.reasm_device(wide.data, offs, caps, n, 1, summary, layers, ml, info, stream)
        torch.cuda.synchronize(DEV)
        assert_equal_info(info.cpu().numpy().view(abi.REASM_DTYPE)[:n], want[:n], f"reasm {st.name}")
        for csum in (False, True):
            o2 = abi.make_opts(0, 8, csum, ml)
            summary.zero_(), layers.zero_(), info.fill_(0xAB)
            engine.parse_reasm_device(wide.data, offs, caps, n, 1, o2, summary, layers, info, stream)
            torch.cuda.synchronize(DEV)
            s, lay = oracle.oracle_parse(st.compact, o2)
            oracle.compare_exact(summary.cpu().numpy().view(abi.SUMMARY_DTYPE), layers.cpu().numpy().view(abi.LAYER_DTYPE)
                                 .reshape(n, ml), s, lay)
            assert_equal_info(info.cpu().numpy().view(abi.REASM_DTYPE)[:n], want[:n], f"fused reasm {st.name}")
        specs = specs_for(st.compact, 1)
        spec = specs[min(3, len(specs) - 1)]
        got = _filter_run(engine, wide.data, offs, caps, n, spec)
        small = _filter_run(engine, *to_device(st.compact, DEV), n, spec)
        assert np.array_equal(got[0], small[0]) and got[1] == small[1] and got[2] == small[2], f"filter {st.name}"
        # the packets the device settles (test_filter.device_finishable), from the wide source, against the restatement's
        # worker: matched[], the counters, and the flow table (key: hash5 under bit 32; first: ~sequence number of the
        # flow's first matching packet)
        s, lay = oracle.oracle_parse(st.compact, FILTER_OPTS)
        idx = np.nonzero(oracle.stats_settled(st.compact, s, lay)[0])[0]
        assert len(idx) >= n - 16, st.name
        sub = PacketBatch(st.compact.data, st.compact.offsets[idx].copy(), st.compact.caplens[idx].copy())
        s, lay = oracle.oracle_parse(sub, FILTER_OPTS)
        flows: dict = {}
        om, ost = oracle.oracle_filter(sub, s, lay, spec, flows)
        it = torch.from_numpy(idx).to(DEV)
        gm, gtable, gstats = _filter_run(engine, wide.data, offs[it], caps[it], len(idx), spec)
        assert np.array_equal(gm, om), f"filter {st.name}"
        gst = dict(zip(abi.STATS_FIELDS, gstats))
        compare_stats(gst, ost)
        assert gst["needs_host_count"] == ost["needs_host_count"] == 0
        first = {}
        for i in np.nonzero(om)[0]:
            first.setdefault(int(s["hash5"][i]), int(i))
        assert set(first) == set(flows)
        assert gtable == {(1 << 32) | h: ~(SEQ_BASE + i) for h, i in first.items()}, f"filter flow table {st.name}"
        matched_total += int(om.sum())
    assert matched_total > len(wide.stages)


def _rules(st, seed):
    """A keep mask and flags records, a bucket column and key records for a stage; the bad descriptors all chosen."""
    rng = np.random.default_rng(seed)
    n = st.n
    dead = np.array([d.dead == cc.DEAD_BAD_DESC for d in st.descs])
    strad = np.array([d.k is not None for d in st.descs])
    keep = (rng.random(n) < 0.6) | dead | strad
    rec = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    fl = rec[:, abi.FLAGS_OFFSET].astype(np.uint16) | (rec[:, abi.FLAGS_OFFSET + 1].astype(np.uint16) << 8)
    force = (dead | strad) & ((fl & 0x0101) == 0)
    rec[force, abi.FLAGS_OFFSET] |= 1
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    return keep.astype(np.uint8), rec.reshape(-1), keys, int(dead.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("snaplen", [0, 60])
def test_gpu_wide_select_and_steer_sources(engine, wide_mis, snaplen):
    """select (keep mask and flags mode) and steer (K = 3, bucket column and key mode) from the wide source into small
    outputs: whole buffers equal to the reference's over the compact batch, the bad descriptors counted."""
    wide = get_wide(wide_mis)
    bad_seen = 0
    for j, st in enumerate(wide.stages):
        offs, caps = put(wide, st)
        src = (wide.data, offs, caps, wide.lay.data_len)
        keep, rec, keys, n_bad = _rules(st, j)
        b = st.compact
        c = sc.Case(st.name, b.data, b.offsets, b.caplens, keep=keep, snaplen=snaplen, out_misalign=j % 16)
        for case in (c, replace(c, keep=None, flags=rec, flags_stride=32, flags_any=0x0101)):
            want = sc.run_reference(case)
            sc.assert_same(sc.run_device(engine, case, DEV, source=src), want, f"select {st.name}")
            assert int(want.totals[abi.SEL_BAD_DESC]) == n_bad, st.name
        t = tc.Case(st.name, b.data, b.offsets, b.caplens, n_buckets=3, snaplen=snaplen, out_misalign=(j + 7) % 16,
                    bucket=(keys % 3).astype(np.uint8))
        for case in (t, tc.with_keys(t, keys, 16, 4)):
            want = tc.run_reference(case)
            tc.assert_same(tc.run_device(engine, case, DEV, source=src), want, f"steer {st.name}")
            assert int(want.totals[abi.STEER_BAD_DESC]) == n_bad and int(want.totals[abi.STEER_OVERFLOW]) == 0, st.name
        bad_seen += n_bad
    assert bad_seen >= 10


# ---------------------------------------------------------------- GPU: the host path past 2^32
HUGE_PAGE = 2 * MIB


def _host_map():
    """2^32 + 2^27 bytes of anonymous private memory, committed page by page as it is touched."""
    size = wc.RAW_BYTES
    try:
        mm = mmap.mmap(-1, size, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS)
        a = np.frombuffer(mm, dtype=np.uint8)
        a[LINE] = 1  # the first touch
    except (OSError, MemoryError, ValueError) as e:
        pytest.fail(f"no host memory for an anonymous map of {size} bytes (lazily committed; under 64 MiB is touched): {e}")
    return mm, a


@pytest.mark.gpu
def test_gpu_wide_host_path(engine):
    """pcppx_parse_batch_host over a pageable host batch whose offsets pass 2^32: a packed run of more than 8192 packets
    across the line (copied straight from the caller's bytes) and the scattered tiles of the stages (gathered packet by
    packet into staging, offsets rebased): the records of the device path over the same packets in a small buffer."""
    from pcapplusplus_amd.engine import parse_on_device

    assert_no_wide_source("the host path test")
    mm, a = _host_map()
    huge = set([LINE // HUGE_PAGE])  # (the first touch)

    def write(off: int, b: np.ndarray) -> None:
        """a[off : off + len(b)] = b, after checking what the write commits: every 2 MiB region touched so far counted
        whole (the most a touch can commit, with transparent huge pages), under 64 MiB."""
        huge.update(range(off // HUGE_PAGE, (off + len(b) - 1) // HUGE_PAGE + 1))
        assert len(huge) * HUGE_PAGE < 64 * MIB, f"the host test would commit {len(huge)} x 2 MiB"
        a[off:off + len(b)] = b

    try:
        lay = wc.layout(0x7F00_8000_0000, 0)  # no device address here: the second line at 2^31 is only a place to be
        opts = abi.make_opts(0, 8, True, 12)
        # (a) the direct run
        pkts, _ = cc.s1_packets()
        run = [pkts[k % len(pkts)] for k in range(9000)]
        total = sum(len(p.data) for p in run)
        pos = LINE - total // 2 - 3
        offs, small_offs, chunks, spos = [], [], [], 0
        for p in run:
            write(pos, np.frombuffer(p.data, np.uint8))
            offs.append(pos)
            small_offs.append(spos)
            chunks.append(p.data)
            pos += len(p.data)
            spos += len(p.data)
        caps = np.array([len(p.data) for p in run], np.uint32)
        woffs = np.array(offs, np.uint64)
        assert len(run) >= 8192 and woffs[0] < LINE < woffs[-1] and ((woffs < LINE) & (woffs + caps > LINE)).sum() == 1
        small = PacketBatch(np.frombuffer(b"".join(chunks) + bytes(16), np.uint8).copy(), np.array(small_offs, np.uint64), caps)
        h = engine.parse_host(PacketBatch(a, woffs, caps), opts)
        d = parse_on_device(engine, small, opts)
        oracle.compare_exact(h[0], h[1], d[0], d[1])
        o = oracle.oracle_parse(small, opts)
        oracle.compare_exact(h[0], h[1], o[0], o[1])
        # (b) scattered tiles: every stage (the last tile of a batch is a run that ends it: copied directly as well)
        for st in wc.stages(lay):
            for off, ext in st.extents:
                write(off, ext)
            h = engine.parse_host(PacketBatch(a[:lay.data_len], st.offsets, st.caplens), opts)
            d = parse_on_device(engine, st.compact, opts)
            oracle.compare_exact(h[0], h[1], d[0], d[1])
            check_against_python(st.case_batch(), h[0][st.known()], f"host path {st.name}")
    finally:
        del a
        try:
            mm.close()
        except BufferError:
            pass


# ---------------------------------------------------------------- GPU: outputs past 2^32
def _slabs(total: int, row: int, limit: int = 256 * MIB):
    """Row ranges [r0, r1) of `total` rows of `row` bytes, each slab under `limit` bytes."""
    per = max(1, limit // max(row, 1))
    return [(r0, min(r0 + per, total)) for r0 in range(0, total, per)]


def _all_fill(t, what: str, fill: int = sc.FILL) -> None:
    for lo in range(0, t.numel(), 512 * MIB):
        assert bool((t[lo:lo + 512 * MIB] == fill).all()), f"{what}: bytes in [{lo}, {lo + 512 * MIB}) were written"


class PeriodRun:
    """R repetitions of a period on the device and output buffers of 0xA5 for select / steer."""

    def __init__(self, p: wc.Period, R: int, data_cap: int, mis: int = 0, on_line: bool = False, index_only: bool = False):
        import torch

        assert_no_wide_source("the destination of a period run")
        self.p, self.R, self.n, self.cap, self.mis = p, R, R * wc.P, data_cap, mis
        up = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
        self.block = up(p.block)
        self.offsets = up(p.offsets.view(np.int64)).repeat(R)
        self.caplens = up(p.caplens.view(np.int32)).repeat(R)
        self.rule = up(p.keep if p.keep is not None else p.bucket).repeat(R)
        one = period_reference(p, 1)
        self.one, self._exp = one, None
        self.groups = period_groups(p, one)
        self.maxp = R * sum(g[1] for g in self.groups)
        self.S = sum(g[3] for g in self.groups)
        self.d_raw = self.d_data = None
        if not index_only:
            extra = 34 * MIB if on_line else 0
            size = 16 + mis + data_cap + sc.PAD_BYTES + extra
            try:
                self.d_raw = torch.full((size,), sc.FILL, dtype=torch.uint8, device=DEV)
            except Exception as e:
                pytest.fail(f"cannot allocate the destination of {size} bytes (data_cap {data_cap}): {e}")
            self.front = 16 + mis
            if on_line:  # the address line of the destination inside the written region, away from its ends and from 2^32
                lay = wc.layout(self.d_raw.data_ptr(), mis, size)
                self.front = lay.pad
                assert lay.data_len >= data_cap + sc.PAD_BYTES and lay.addr_line + 16 * MIB <= R * self.S
                self.addr_line = lay.addr_line
            self.d_data = self.d_raw[self.front:]
            assert self.d_data.data_ptr() % 16 == mis
        self.d_off = up(np.full(self.maxp + sc.PAD_ENTRIES, tc.F64, np.uint64).view(np.int64))
        self.d_cap = up(np.full(self.maxp + sc.PAD_ENTRIES, tc.F32, np.uint32).view(np.int32))
        self.d_idx = up(np.full(self.maxp + sc.PAD_ENTRIES, tc.F32, np.uint32).view(np.int32))
        self.d_tot = up(np.full(8, tc.F64, np.uint64).view(np.int64))
        if p.keep is None:
            self.d_first = up(np.full(p.K + 1 + sc.PAD_ENTRIES, tc.F32, np.uint32).view(np.int32))
            self.d_pos = up(np.full(p.K + 1 + sc.PAD_ENTRIES, tc.F64, np.uint64).view(np.int64))

    def launch(self, engine) -> None:
        import torch

        p = self.p
        stream = torch.cuda.current_stream(DEV).cuda_stream
        if p.keep is not None:
            engine.select_device(self.block, self.offsets, self.caplens, self.n, 1,
                                 abi.make_select_spec(keep=abi.ptr(self.rule)), self.d_off, self.d_cap, self.d_tot,
                                 self.maxp, self.d_data, self.cap, self.d_idx, stream)
        else:
            engine.steer_device(self.block, self.offsets, self.caplens, self.n, 1,
                                abi.make_steer_spec(bucket=abi.ptr(self.rule), n_buckets=p.K), self.d_off, self.d_cap,
                                self.d_first, self.d_pos, self.d_tot, self.maxp, self.d_data, self.cap, self.d_idx, stream)
        torch.cuda.synchronize(DEV)

    def totals(self) -> list[int]:
        return [int(x) for x in self.d_tot.cpu().numpy().view(np.uint64)]

    def expected(self) -> dict:
        if self._exp is None:
            self._exp = expected_repeats(self.p, self.one, self.R)
        return self._exp

    def check_entries(self, written: int | None = None) -> None:
        """offsets / caplens / index: the first `written` entries (None: all) as expected, the rest still the fill."""
        exp = self.expected()
        w = self.maxp if written is None else written
        for f, t, dt, fill in (("offsets", self.d_off, np.uint64, tc.F64), ("caplens", self.d_cap, np.uint32, tc.F32),
                               ("index", self.d_idx, np.uint32, tc.F32)):
            got = t.cpu().numpy().view(dt)
            bad = np.nonzero(got[:w] != exp[f][:w])[0]
            assert len(bad) == 0, (f, len(bad), "first at", int(bad[0]), int(got[bad[0]]), int(exp[f][bad[0]]))
            assert (got[w:] == fill).all(), (f, "entries past the written ones were touched")

    def check_buckets(self) -> None:
        exp = self.expected()
        K = self.p.K
        gf, gp = self.d_first.cpu().numpy().view(np.uint32), self.d_pos.cpu().numpy().view(np.uint64)
        assert np.array_equal(gf[:K + 1], exp["bucket_first"]) and (gf[K + 1:] == tc.F32).all()
        assert np.array_equal(gp[:K + 1], exp["bucket_pos"]) and (gp[K + 1:] == tc.F64).all()

    def check_bytes(self, written_bytes: int | None = None) -> None:
        """out.data: every repetition of every group equal to the period's bytes (select: up to written_bytes), 0xA5
        everywhere else, the bytes in front of out.data included."""
        import torch

        pos = 0
        for _, _, at, nb in self.groups:
            if nb:
                want = torch.from_numpy(self.one.data[at:at + nb].copy()).to(DEV)
                rows = self.R if written_bytes is None else max(0, min(self.R, (written_bytes - pos) // nb))
                for r0, r1 in _slabs(rows, nb):
                    got = self.d_data[pos + r0 * nb: pos + r1 * nb].view(r1 - r0, nb)
                    eq = (got == want[None, :]).all(dim=1)
                    if not bool(eq.all()):
                        r = r0 + int(torch.nonzero(~eq)[0])
                        c = int(torch.nonzero(got[r - r0] != want)[0])
                        raise AssertionError(f"out.data differs in repetition {r} at byte {pos + r * nb + c} "
                                             f"(destination address {self.d_data.data_ptr() + pos + r * nb + c:#x})")
                if written_bytes is not None and rows < self.R:  # the partial repetition at the capacity
                    rest = written_bytes - pos - rows * nb
                    assert 0 <= rest < nb
                    assert bool((self.d_data[pos + rows * nb: written_bytes] == want[:rest]).all())
            pos += self.R * nb
        end = pos if written_bytes is None else written_bytes
        _all_fill(self.d_data[end:], "after the output")
        _all_fill(self.d_raw[:self.front], "in front of out.data")


def _period_sizes(K: int):
    p = wc.period(K)
    S = sum(p.sums())
    return p, S, wc.repeats(S)


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [0, 9])
def test_gpu_select_output_past_4gib(engine, mis):
    """pcppx_select_device writing 4.25 GiB: byte positions, block bases and out.offsets past 2^32, the destination's own
    address line inside the written region, every repetition on another destination alignment."""
    p, S, R = _period_sizes(0)
    run = PeriodRun(p, R, R * S, mis, on_line=True)
    assert run.n > 3 * 256 * 1024 and R * S >= LINE + (1 << 28) and 16 * MIB <= run.addr_line <= LINE - 16 * MIB
    run.launch(engine)
    assert run.totals()[:5] == [run.maxp, R * S, run.maxp, R * S, 0]
    run.check_entries()
    run.check_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("K,mis", [(3, 0), (3, 9), (64, 0), (64, 9)])
def test_gpu_steer_output_past_4gib(engine, K, mis):
    """pcppx_steer_device writing 4.25 GiB: per-bucket scans over thousands of blocks, block byte prefixes, bucket_pos and
    out.offsets past 2^32."""
    p, S, R = _period_sizes(K)
    run = PeriodRun(p, R, R * S, mis, on_line=True)
    assert run.n > 3 * 256 * 1024 and R * S >= LINE + (1 << 28)
    run.launch(engine)
    dropped = R * int((p.bucket >= K).sum())
    assert run.totals()[:5] == [run.maxp, R * S, dropped, 0, 0]
    run.check_buckets()
    if K == 3:  # a bucket of more than 2^32 bytes, and a bucket that starts past 2^32
        pos = run.d_pos.cpu().numpy().view(np.uint64)
        assert int(pos[2]) >= LINE and int(pos[2]) - int(pos[1]) >= LINE
    run.check_entries()
    run.check_bytes()


def _select_prefix(run: PeriodRun, cap: int) -> tuple[int, int]:
    """(written packets, written bytes): the longest prefix of the kept packets that fits cap bytes."""
    S = run.S
    q = cap // S
    assert q < run.R
    _, cnt, _, _ = run.groups[0]
    ends = np.cumsum(run.one.caplens[:cnt].astype(np.int64))
    j = int(np.searchsorted(ends, cap - q * S, side="right"))  # the first kept packet that does not fit closes the output
    return q * cnt + j, q * S + (int(ends[j - 1]) if j else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("short", ["line", "one"])
def test_gpu_select_capacity_at_the_line(engine, short):
    """data_cap = 2^32 - 1 against 2^32 + a bytes selected (a 32-bit comparison says "fits"), and data_cap one byte short
    of everything: WRITTEN_* is the longest prefix that fits, SELECTED_* the whole, nothing past WRITTEN_BYTES touched."""
    p, S, R = _period_sizes(0)
    cap = LINE - 1 if short == "line" else R * S - 1
    run = PeriodRun(p, R, cap)
    wp, wb = _select_prefix(run, cap)
    assert (R * S) % LINE < cap and wb <= cap < R * S
    if short == "one":  # exactly the last kept non-empty packet is not written (and the empty ones behind it)
        _, cnt, _, _ = run.groups[0]
        lens = run.one.caplens[:cnt]
        last = int(np.nonzero(lens)[0][-1])
        assert (wp, wb) == (run.maxp - (cnt - last), R * S - int(lens[last]))
    run.launch(engine)
    assert run.totals()[:5] == [run.maxp, R * S, wp, wb, 0]
    run.check_entries(wp)
    run.check_bytes(wb)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 64])
@pytest.mark.parametrize("short", ["line", "one"])
def test_gpu_steer_capacity_at_the_line(engine, K, short):
    """All or nothing at data_cap = 2^32 - 1 and one byte short: the overflow verdict set, totals and bucket bounds exact,
    not a byte of data / offsets / caplens / index touched."""
    p, S, R = _period_sizes(K)
    cap = LINE - 1 if short == "line" else R * S - 1
    assert (R * S) % LINE < cap < R * S
    run = PeriodRun(p, R, cap)
    run.launch(engine)
    assert run.totals()[:5] == [run.maxp, R * S, R * int((p.bucket >= K).sum()), 0, 1]
    run.check_buckets()
    run.check_entries(0)
    _all_fill(run.d_raw, "steer overflow: out.data")


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 64])
def test_gpu_steer_index_only_at_full_n(engine, K):
    p, S, R = _period_sizes(K)
    run = PeriodRun(p, R, 0, index_only=True)
    run.launch(engine)
    assert run.totals()[:5] == [run.maxp, R * S, R * int((p.bucket >= K).sum()), 0, 0]
    run.check_buckets()
    run.check_entries()
