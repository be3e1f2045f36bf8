"""Time of pcppx_tlsfp_device on a device-resident batch, beside the device parse of the same batch and the single-core
time of pcppx_tlsfp_reference.

  python tools/bench_tlsfp.py [packets] [launches] [out.json] [only-share]

Workload: config-3 IMIX (64 / 512 / 1500 B at 7:4:1, 25 % VLAN, 30 % IPv6), `packets` of it (1M by default), of which
a share of 0.1 %, 1 %, 10 % and 100 % (evenly spread) is replaced by TLS hello packets: 64 different ClientHellos and
ServerHellos in turn, of ~100-300 text bytes. The batch is resident in HBM and parsed once (summary, FIXED layers);
both kinds are fingerprinted, with the text and the dispositions written; the buffers are sized by a call with
max_recs = 0, as a caller would.
Method: after 3 warm-up launches, `launches` (>= 50) launches, each between its own pair of HIP events on the launch
stream, nothing else running on the device; the median, the minimum and the maximum of the per-launch times are given.
The parse of the same batch is timed the same way in the same process. pcppx_tlsfp_reference runs once on one core
over the same batch and records. There is no earlier implementation to compare with: the file holds what was measured.
Prints one JSON line (and writes it to out.json when given).
"""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, synth, tlsfp  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402
from pcapplusplus_amd.pcap import PacketBatch, from_packets  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
out_path = (sys.argv[3] if len(sys.argv) > 3 else None) or None
only = float(sys.argv[4]) if len(sys.argv) > 4 else None
ML = 8
SHARES = (0.001, 0.01, 0.1, 1.0)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)


def hello_pool() -> PacketBatch:
    """64 hello packets: ClientHellos with 8..39 cipher suites and the usual extensions, ServerHellos of TLS 1.2 / 1.3."""
    out = []
    for k in range(32):
        exts = tlsfp.ext(0, b"\0\x0e\0\0\x0bexample.com") + tlsfp.ext(23) + tlsfp.ext(65281, b"\0") + \
            tlsfp.groups_ext([0x0A0A, 29, 23, 24, 25][:2 + k % 4]) + tlsfp.formats_ext([0]) + tlsfp.ext(35) + \
            tlsfp.ext(16, b"\0\x0c\x02h2\x08http/1.1") + tlsfp.ext(5, b"\x01\0\0\0\0") + tlsfp.ext(13, bytes(20)) + \
            tlsfp.ext(51, bytes(38)) + tlsfp.ext(45, b"\x01\x01") + tlsfp.ext(43, b"\x06\x0a\x0a\x03\x04\x03\x03")
        ciphers = [0x1A1A, 0x1301, 0x1302, 0x1303] + [0xC02B + j for j in range(4 + k)]
        out.append(tlsfp.tcp_packet(tlsfp.record(tlsfp.client_hello(ciphers, exts, sid=bytes(32))), k, v6=k % 3 == 0))
        sx = tlsfp.ext(43, b"\x03\x04") + tlsfp.ext(51, bytes(36)) if k % 2 else \
            tlsfp.ext(65281, b"\0") + tlsfp.ext(11, b"\x01\0") + tlsfp.ext(35) + tlsfp.ext(16, b"\0\x03\x02h2")
        out.append(tlsfp.tcp_packet(tlsfp.record(tlsfp.server_hello(0xC02B + k, sx, sid=bytes(32))), k, True,
                                    v6=k % 3 == 0))
    return from_packets(out)


def with_hellos(b: PacketBatch, pool: PacketBatch, share: float) -> PacketBatch:
    """b with every (1 / share)-th packet replaced by one of the pool's (its bytes appended behind b's)."""
    at = np.unique((np.arange(int(round(b.n * share))) / share).astype(np.int64).clip(0, b.n - 1))
    base = len(b.data)
    offs, caps = b.offsets.copy(), b.caplens.copy()
    which = np.arange(len(at)) % pool.n
    offs[at] = pool.offsets[which] + np.uint64(base)
    caps[at] = pool.caplens[which]
    return PacketBatch(np.concatenate([b.data, pool.data]), offs, caps, b.linktype)


def per_launch(fn, reps: int) -> list:
    pairs = []
    for _ in range(reps):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        z.record(st)
        pairs.append((a, z))
    torch.cuda.synchronize()
    return [a.elapsed_time(z) for a, z in pairs]


def stats(ms: list) -> dict:
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


imix, pool = synth.config(3, n), hello_pool()
results = []
for share in SHARES:
    if only is not None and only != share:
        continue
    b = with_hellos(imix, pool, share)
    data, offsets, caplens = to_device(b, dev)
    summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
    opts = abi.make_opts(0, 8, False, ML)
    parse = lambda: eng.parse_device(data, offsets, caplens, n, b.linktype, opts, summary, layers,  # noqa: E731
                                     st.cuda_stream)
    parse()
    spec = abi.make_tlsfp_spec(True, True)
    totals = torch.zeros(abi.TLSFP_TOTALS, dtype=torch.int64, device=dev)
    eng.tlsfp_device(data, offsets, caplens, n, b.linktype, layers, ML, spec,
                     torch.empty(40, dtype=torch.uint8, device=dev), totals, 0, stream=st.cuda_stream, summary=summary)
    torch.cuda.synchronize()
    need = abi.tlsfp_totals_dict(totals.cpu().numpy().view(np.uint64))
    k, nb = need["client_n"] + need["server_n"], need["text_bytes"]
    recs = torch.empty(max(k, 1) * 40, dtype=torch.uint8, device=dev)
    text = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    run = lambda: eng.tlsfp_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, recs, totals, k,  # noqa: E731
                                   text, nb, disp, st.cuda_stream, summary=summary)
    for _ in range(3):
        run()
        parse()
    torch.cuda.synchronize()
    tot = abi.tlsfp_totals_dict(totals.cpu().numpy().view(np.uint64))
    assert tot["overflow"] == 0 and tot["candidates"] == k == len(np.unique((np.arange(int(round(n * share))) / share)
                                                                            .astype(np.int64).clip(0, n - 1)))
    t_ms, p_ms = per_launch(run, launches), per_launch(parse, launches)
    # the same batch and records through the host reference, one core
    h_sum, h_lay = summary.cpu().numpy(), layers.cpu().numpy()
    h_recs, h_text = np.empty(max(k, 1) * 40, np.uint8), np.empty(nb + 64, np.uint8)
    h_disp, h_tot = np.empty(n, np.uint8), np.zeros(abi.TLSFP_TOTALS, np.uint64)
    hb = abi.Batch(b.data.ctypes.data, b.offsets.ctypes.data, b.caplens.ctypes.data, len(b.data), n, b.linktype, 0)
    ho = abi.Tlsfps(h_recs.ctypes.data, h_text.ctypes.data, nb, h_disp.ctypes.data, k, 0, h_tot.ctypes.data)
    t0 = time.perf_counter()
    abi.tlsfp_reference(hb, abi.Records(h_sum.ctypes.data, h_lay.ctypes.data), ML, spec, ho)
    ref_ms = (time.perf_counter() - t0) * 1e3
    same = bool((recs.cpu().numpy()[:k * 40] == h_recs[:k * 40]).all() and (text.cpu().numpy()[:nb] == h_text[:nb]).all()
                and (disp.cpu().numpy() == h_disp).all())
    med = statistics.median(t_ms)
    results.append({"hello_share": share, "packets": n, "hellos": k, "text_bytes": nb, "tlsfp": stats(t_ms),
                    "Mpps": round(n / med / 1e3, 1), "hellos_per_us": round(k / med / 1e3, 2), "parse": stats(p_ms),
                    "tlsfp_over_parse": round(med / statistics.median(p_ms), 3),
                    "reference_one_core_ms": round(ref_ms, 2), "device_equals_reference": same})
    del data, offsets, caplens, summary, layers, recs, text, disp
    torch.cuda.empty_cache()
line = json.dumps({"kernel": "tlsfp (plan + bases + emit)", "launches_per_case": launches, "warmup_launches": 3,
                   "timing": "one HIP event pair per launch, median of the launches", "cases": results})
print(line)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(line + "\n")
eng.close()
