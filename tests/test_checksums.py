"""The checksum path of the parse kernels against an independent RFC 1071 reference (tests/checksum_cases.py).

The span stream with its wave prefix scan, the whole-chunk sums of tiles that cannot stream, the masked edge chunks,
range_residue's LDS -> HBM hand-over, the arithmetic mod 65535 and the byte swap for odd start addresses are reached
by the other GPU tests only with 4-aligned packets, fixed wrong stored checksums and residues hit by chance. Here every
packet's four checksum fields and four verdict bits are computed in plain Python from offsets the generator knows,
for every start alignment, the residues where mod-65535 arithmetic and end-around carry differ, header stacks across
the window ends, and batch shapes (partial tiles, dead descriptors, sparse tiles, the stream criterion's two sides,
sums past 2^32, shared bytes). The CPU test pins the restatement and the reference Packet++ to the same values.
"""
from __future__ import annotations

import numpy as np
import pytest

import checksum_cases as cc
import oracle
from pcapplusplus_amd import abi

CSUM_BITS = abi.F_IP_CSUM | abi.F_IP_CSUM_OK | abi.F_L4_CSUM | abi.F_L4_CSUM_OK
DEAD_FLAGS = {cc.DEAD_BAD_DESC: abi.F_BAD_DESC, cc.DEAD_EMPTY: 0, cc.DEAD_OVERSIZE: abi.F_OVERSIZE}
_restated: dict[str, tuple] = {}


def opts_for(window: int = abi.WINDOW_DEFAULT, layout: int = abi.LAYOUT_FIXED) -> abi.Opts:
    return abi.make_opts(0, 8, True, 12, window, layout)


def restated(cb: cc.CaseBatch):
    """The restatement's records of a case batch (the window is a speed choice: one parse serves every launch)."""
    if cb.name not in _restated:
        _restated[cb.name] = oracle.oracle_parse(cb.batch, opts_for())
    return _restated[cb.name]


def expected_bits(e: np.ndarray) -> np.ndarray:
    return (e["live"] * abi.F_L4_CSUM + e["l4_ok"] * abi.F_L4_CSUM_OK + e["has_ip4"] * abi.F_IP_CSUM +
            e["ip_ok"] * abi.F_IP_CSUM_OK).astype(np.uint16)


def check_flag_bits(cb: cc.CaseBatch, flags: np.ndarray, what: str) -> None:
    """The four checksum verdict bits (and the trailer bit, and a dead descriptor's whole flag word) on every packet."""
    e = cb.expect
    want = expected_bits(e)
    bad = np.nonzero((flags & CSUM_BITS) != want)[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError(f"{what}: checksum flag bits differ on {len(bad)} packets; first {cb.describe(i)}: "
                             f"got {int(flags[i]) & CSUM_BITS:#06x} want {int(want[i]):#06x}")
    bad = np.nonzero(e["live"] & (((flags & abi.F_TRAILER) != 0) != e["trailer"]))[0]
    assert not len(bad), f"{what}: trailer bit differs; first {cb.describe(int(bad[0]))}"
    for kind, fl in DEAD_FLAGS.items():
        bad = np.nonzero((e["dead"] == kind) & (flags != fl))[0]
        assert not len(bad), f"{what}: dead descriptor flags {int(flags[bad[0]]):#06x}; first {cb.describe(int(bad[0]))}"


def check_against_python(cb: cc.CaseBatch, s: np.ndarray, what: str) -> None:
    """Checksum fields and verdict bits of summary records against the Python reference, every packet."""
    e = cb.expect
    for f, m in (("l4_calc", e["live"]), ("l4_stored", e["live"]), ("ip_calc", e["has_ip4"]), ("ip_stored", e["has_ip4"])):
        got = s[f.replace("_", "_csum_")]
        bad = np.nonzero(m & (got != e[f]))[0]
        if len(bad):
            i = int(bad[0])
            raise AssertionError(f"{what}: {f} differs on {len(bad)} packets; first {cb.describe(i)}: "
                                 f"got {int(got[i]):#06x} want {int(e[f][i]):#06x}")
    check_flag_bits(cb, s["flags"], what)
    dead = e["dead"] != 0
    assert (s["n_layers"][dead] == 0).all(), f"{what}: a dead descriptor has layers"


def check_layout(cb: cc.CaseBatch) -> None:
    """The tiles meant to stream (or not) do, by the kernel's criterion emax - smin <= 2 * wire + 65536 over the
    descriptors; S4d sits exactly on it (tile 0) and one 16-B chunk past it (tile 1)."""
    if cb.stream is not None:
        got = [cc.tile_streams(cb.batch, t) for t in range((cb.batch.n + cc.TILE - 1) // cc.TILE)]
        assert got == cb.stream, (cb.name, got)
    if cb.name.startswith("S4d"):
        for t, extra in ((0, 0), (1, 16)):
            smin, emax, wire = cc.tile_span(cb.batch, t)
            assert wire == cb.meta["wire"] and emax - smin == 2 * wire + 65536 + extra, (t, smin, emax, wire)
            gaps = np.diff(np.sort(cb.batch.offsets[t * 64:(t + 1) * 64].astype(np.int64)))
            assert (gaps > 4096).sum() == 1  # a single gap


@pytest.mark.parametrize("name", list(cc.SETS))
def test_checksum_cases_pin_restatement_and_reference(name):
    """Every set: the Python reference's four fields and four verdict bits equal the restatement's on every packet, and
    the restatement's records pass the engine contract against the reference Packet++ where it is built. No case is
    excused: every packet carries an L4 checksum and none is left to the host."""
    total = 0
    for cb in cc.SETS[name]():
        check_layout(cb)
        o = restated(cb)
        live = cb.expect["live"]
        fl = o[0]["flags"]
        assert ((fl[live] & abi.F_L4_CSUM) != 0).all(), cb.describe(int(np.nonzero(live & ((fl & abi.F_L4_CSUM) == 0))[0][0]))
        assert ((fl[live] & abi.F_NEEDS_HOST) == 0).all(), cb.describe(int(np.nonzero(live & ((fl & abi.F_NEEDS_HOST) != 0))[0][0]))
        check_against_python(cb, o[0], "restatement")
        if oracle.ref_available():
            sub = cb.alone or cb  # the reference harness takes no dead descriptors
            so = restated(sub)
            r = oracle.ref_parse(sub.batch, opts_for())
            check_against_python(sub, r[0], "reference Packet++")
            oracle.compare_engine_to_reference(so[0], so[1], r[0], r[1])
        total += int(live.sum())
    assert total >= {"S1": 6784, "S2": 1000, "S3": 3000, "S4": 1000}[name]


# ---------------------------------------------------------------- GPU
def device_parse(engine, batch, opts, kernel: int):
    """kernel 0: the product tile kernel (libpcppx.so); 1: the lane-per-packet cross-check kernel of the tools-only A/B
    library. The data pointer is 16-B aligned on every launch, so a packet's offset mod 16 is its address mod 16."""
    import torch

    from pcapplusplus_amd.engine import records_from_device, to_device

    data, offsets, caplens = to_device(batch)
    assert data.data_ptr() % 16 == 0
    n = batch.n
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=data.device)
    layers = torch.zeros(max(n * opts.max_layers, 1) * 8, dtype=torch.uint8, device=data.device)
    stream = torch.cuda.current_stream(data.device).cuda_stream
    if kernel == 0:
        engine.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, stream)
    else:
        from tools import ab

        ab.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, stream, ab.LANE)
    torch.cuda.synchronize(data.device)
    return records_from_device(summary, layers, n, opts.max_layers)


def gpu_set(engine, name: str, window: int, kernel: int) -> None:
    opts = opts_for(window)
    for cb in cc.SETS[name]():
        check_layout(cb)
        g = device_parse(engine, cb.batch, opts, kernel)
        o = restated(cb)
        oracle.compare_exact(g[0], g[1], o[0], o[1])
        check_against_python(cb, g[0], "device")
        sub, gs = cb, g
        if cb.alone is not None:  # live packets beside dead descriptors: the records of the same packets parsed alone
            sub = cb.alone
            gs = device_parse(engine, sub.batch, opts, kernel)
            live = cb.meta["live"]
            oracle.compare_exact(g[0][live], g[1][live], gs[0], gs[1])
            check_against_python(sub, gs[0], "device")
        if oracle.ref_available():
            r = oracle.ref_parse(sub.batch, opts)
            oracle.compare_engine_to_reference(gs[0], gs[1], r[0], r[1])


WINDOWS = pytest.mark.parametrize("window", [abi.WINDOW_DEFAULT, abi.WINDOW_DEEP], ids=["default", "deep"])
KERNELS = pytest.mark.parametrize("kernel", [0, 1], ids=["tile", "lane"])


@pytest.mark.gpu
@WINDOWS
@KERNELS
def test_gpu_checksums_length_x_alignment(engine, window, kernel):
    """S1: payload lengths 0..96, 127..129, 255..257, 1459..1461 x four families x 16 start alignments, IHL 5..15."""
    gpu_set(engine, "S1", window, kernel)


@pytest.mark.gpu
@WINDOWS
@KERNELS
def test_gpu_checksums_residue_edges(engine, window, kernel):
    """S2: computed checksums steered to 0x0000 / 0x0001 / 0xFFFE / 0x00FF / 0xFF00 / 0x8000 (UDP's 0 -> 0xFFFF) and
    the stored 0x0000 / 0xFFFF aliases that must not verify, at even and odd addresses."""
    gpu_set(engine, "S2", window, kernel)


@pytest.mark.gpu
@WINDOWS
@KERNELS
def test_gpu_checksums_chain_shapes(engine, window, kernel):
    """S3: Ethernet padding, truncated captures, VLAN / MPLS / IPv4 options across the window ends, GRE; 16 alignments."""
    gpu_set(engine, "S3", window, kernel)


@pytest.mark.gpu
@WINDOWS
@KERNELS
def test_gpu_checksums_batch_structure(engine, window, kernel):
    """S4: partial tiles, dead descriptors in a streaming tile, sparse tiles, the stream criterion on both sides, sums
    near and past 2^32, descriptors sharing bytes."""
    gpu_set(engine, "S4", window, kernel)


@pytest.mark.gpu
def test_gpu_checksums_other_entry_points(engine):
    """S1 + S2 through the chunked host path and through the bench's launch (PACKED rows + the 16-B brief, no
    summary): the host path's fields and bits, and the brief's verdict bits, equal the Python reference's."""
    from pcapplusplus_amd.engine import parse_on_device_ex

    for name in ("S1", "S2"):
        for cb in cc.SETS[name]():
            o = restated(cb)
            for window in (abi.WINDOW_DEFAULT, abi.WINDOW_DEEP):
                h = engine.parse_host(cb.batch, opts_for(window))
                oracle.compare_exact(h[0], h[1], o[0], o[1])
                check_against_python(cb, h[0], "host path")
                g = parse_on_device_ex(engine, cb.batch, opts_for(window, abi.LAYOUT_PACKED), summary=False, brief=True)
                check_flag_bits(cb, g["brief"]["flags"], "brief")
                for f in abi.BRIEF_DTYPE.names:
                    assert np.array_equal(g["brief"][f], o[0][f]), f
                valid = np.arange(12)[None, :] < o[0]["n_layers"][:, None]
                zero = np.zeros(1, abi.LAYER_DTYPE)
                assert np.where(valid, g["layers"], zero).tobytes() == np.where(valid, o[1], zero).tobytes()
