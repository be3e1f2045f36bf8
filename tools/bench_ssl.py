"""Time of pcppx_ssl_device on a device-resident batch, beside pcppx_tlsfp_device and the device parse of the same batch
and the single-core time of pcppx_ssl_reference.

  python tools/bench_ssl.py [packets] [launches] [out.json]

Workload: config-3 IMIX (64 / 512 / 1500 B at 7:4:1, 25 % VLAN, 30 % IPv6), `packets` of it (1M by default), of which
a share of 1 %, 10 % and 100 % (evenly spread) is replaced by packets on port 443 with a payload, those of the
reference's tls.pcap and of many_protocols_ssl.pcap (tests/golden/ssl) in turn; some two thirds of them start with an
SSL record. The batch is resident in HBM and parsed once (summary, FIXED layers); the spec asks for both hello kinds,
the names and the dispositions written; the buffers are sized by a call without room, as a caller would.
Method: after 3 warm-up launches, `launches` (>= 50) launches, each between its own pair of HIP events on the launch
stream, nothing else running on the device; the median, the minimum and the maximum of the per-launch times are given.
pcppx_tlsfp_device (both kinds, with text) and the parse of the same batch are timed the same way in the same process,
for context. pcppx_ssl_reference runs once on one core over the same batch and records, and the device's output is
compared with its output in every row. There is no earlier implementation to compare with: the file holds what was
measured.
Prints one JSON line (and writes it into out.json when given).
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

from pcapplusplus_amd import abi, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402
from pcapplusplus_amd.pcap import PacketBatch, concat, from_packets, read_pcap  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
out_path = (sys.argv[3] if len(sys.argv) > 3 else None) or None

ML = 8
SHARES = (0.01, 0.1, 1.0)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)


def with_ssl(b: PacketBatch, pool: PacketBatch, share: float) -> PacketBatch:
    """b with every (1 / share)-th packet replaced by one of the pool's (its bytes appended behind b's)."""
    at = np.unique((np.arange(int(round(b.n * share))) / share).astype(np.int64).clip(0, b.n - 1))
    base = len(b.data)
    offs, caps = b.offsets.copy(), b.caplens.copy()
    which = np.arange(len(at)) % pool.n
    offs[at] = pool.offsets[which] + np.uint64(base)
    caps[at] = pool.caplens[which]
    return PacketBatch(np.concatenate([b.data, pool.data]), offs, caps, b.linktype)


def ssl_pool() -> PacketBatch:
    """The captures' packets on an SSL port that carry a payload."""
    golden = ROOT / "tests" / "golden" / "ssl"
    both = concat([read_pcap(golden / "tls.pcap"), read_pcap(golden / "many_protocols_ssl.pcap")])
    keep = [both.packet(i) for i in range(both.n) if both.caplens[i] > 66 and both.packet(i)[12:14] == b"\x08\x00" and
            both.packet(i)[23] == 6 and 443 in (int.from_bytes(both.packet(i)[34:36], "big"),
                                                int.from_bytes(both.packet(i)[36:38], "big"))]
    return from_packets(keep)


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


imix = synth.config(3, n)
pool = ssl_pool()
results = []
for share in SHARES:
    b = with_ssl(imix, pool, share)
    data, offsets, caplens = to_device(b, dev)
    summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
    opts = abi.make_opts(0, 8, False, ML)
    parse = lambda: eng.parse_device(data, offsets, caplens, n, b.linktype, opts, summary, layers,  # noqa: E731
                                     st.cuda_stream)
    parse()
    spec = abi.make_ssl_spec(3)
    totals = torch.zeros(abi.SSL_TOTALS, dtype=torch.int64, device=dev)
    one = torch.empty(40, dtype=torch.uint8, device=dev)
    eng.ssl_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, one, one, totals, 0, 0,
                   stream=st.cuda_stream, summary=summary)
    torch.cuda.synchronize()
    need = abi.ssl_totals_dict(totals.cpu().numpy().view(np.uint64))
    m, k, nb = need["msgs"], need["hellos"], need["name_bytes"]
    msgs = torch.empty(max(m, 1) * 32, dtype=torch.uint8, device=dev)
    hellos = torch.empty(max(k, 1) * 32, dtype=torch.uint8, device=dev)
    names = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    run = lambda: eng.ssl_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, msgs, hellos, totals, m, k,  # noqa: E731
                                 names, nb, disp, st.cuda_stream, summary=summary)
    # pcppx_tlsfp_device on the same batch, sized the same way
    fspec = abi.make_tlsfp_spec(True, True)
    ftot = torch.zeros(abi.TLSFP_TOTALS, dtype=torch.int64, device=dev)
    eng.tlsfp_device(data, offsets, caplens, n, b.linktype, layers, ML, fspec, one, ftot, 0, stream=st.cuda_stream,
                     summary=summary)
    torch.cuda.synchronize()
    fneed = abi.tlsfp_totals_dict(ftot.cpu().numpy().view(np.uint64))
    fk, fnb = fneed["client_n"] + fneed["server_n"], fneed["text_bytes"]
    frecs = torch.empty(max(fk, 1) * 40, dtype=torch.uint8, device=dev)
    ftext = torch.empty(fnb + 64, dtype=torch.uint8, device=dev)
    fdisp = torch.empty(n, dtype=torch.uint8, device=dev)
    tlsfp = lambda: eng.tlsfp_device(data, offsets, caplens, n, b.linktype, layers, ML, fspec, frecs, ftot, fk, ftext,  # noqa: E731
                                     fnb, fdisp, st.cuda_stream, summary=summary)
    for _ in range(3):
        run()
        tlsfp()
        parse()
    torch.cuda.synchronize()
    tot = abi.ssl_totals_dict(totals.cpu().numpy().view(np.uint64))
    assert tot["overflow"] == 0 and tot["msgs"] == m
    t_ms, f_ms, p_ms = per_launch(run, launches), per_launch(tlsfp, launches), per_launch(parse, launches)
    # the same batch and records through the host reference, one core
    h_sum, h_lay = summary.cpu().numpy(), layers.cpu().numpy()
    h_msgs, h_hellos = np.empty(max(m, 1) * 32, np.uint8), np.empty(max(k, 1) * 32, np.uint8)
    h_names, h_disp, h_tot = np.empty(nb + 64, np.uint8), np.empty(n, np.uint8), np.zeros(abi.SSL_TOTALS, np.uint64)
    hb = abi.Batch(b.data.ctypes.data, b.offsets.ctypes.data, b.caplens.ctypes.data, len(b.data), n, b.linktype, 0)
    ho = abi.SslOut(h_msgs.ctypes.data, h_hellos.ctypes.data, h_names.ctypes.data, nb, h_disp.ctypes.data, m, k,
                    h_tot.ctypes.data)
    t0 = time.perf_counter()
    abi.ssl_reference(hb, abi.Records(h_sum.ctypes.data, h_lay.ctypes.data), ML, spec, ho)
    ref_ms = (time.perf_counter() - t0) * 1e3
    same = bool((msgs.cpu().numpy()[:m * 32] == h_msgs[:m * 32]).all() and
                (hellos.cpu().numpy()[:k * 32] == h_hellos[:k * 32]).all() and
                (names.cpu().numpy()[:nb] == h_names[:nb]).all() and (disp.cpu().numpy() == h_disp).all() and
                list(totals.cpu().numpy().view(np.uint64)) == list(h_tot))
    med = statistics.median(t_ms)
    results.append({"ssl_share": share, "packets": n, "messages": m, "hellos": k, "name_bytes": nb,
                    "payload_bytes": tot["payload_bytes"], "host_n": tot["host_n"], "ssl": stats(t_ms),
                    "Gpkt_per_s": round(n / med / 1e6, 3), "messages_per_us": round(m / med / 1e3, 2),
                    "tlsfp": stats(f_ms), "tlsfp_records": fk, "parse": stats(p_ms),
                    "ssl_over_parse": round(med / statistics.median(p_ms), 3),
                    "reference_one_core_ms": round(ref_ms, 2), "device_equals_reference": same})
    del data, offsets, caplens, summary, layers, msgs, hellos, names, disp, frecs, ftext, fdisp
    torch.cuda.empty_cache()
entry = {"kernel": "ssl (plan + bases + emit)", "launches_per_case": launches, "warmup_launches": 3,
         "timing": "one HIP event pair per launch, median of the launches", "cases": results}
print(json.dumps(entry))
if out_path:
    p = Path(out_path)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(entry) + "\n")
eng.close()
assert all(r["device_equals_reference"] for r in results)
