"""Time of pcppx_sip_device on a device-resident batch, beside the device parse of the same batch and the single-core
time of pcppx_sip_reference.

  python tools/bench_sip.py [packets] [launches] [out.json]

Workload: config-3 IMIX (64 / 512 / 1500 B at 7:4:1, 25 % VLAN, 30 % IPv6), `packets` of it (1M by default), of which
a share of 1 % and 100 % (evenly spread) is replaced by SIP packets from pcapplusplus_amd.sip's builders: 4096 distinct
messages -- requests of the 14 methods and responses in turn, every third with an SDP body, four in five on port 5060
over UDP (one in seven of those over TCP), one in five on other ports (the heuristic path). The batch is resident in HBM
and parsed once (summary, FIXED layers); the spec asks for no field records (NONE) or for Call-ID, From, To and CSeq
(WANTED), each with the first line's text and the values (text 3), the dispositions written; the buffers are sized by a
call without room, as a caller would.
Method: after 3 warm-up launches, `launches` (>= 50) launches, each between its own pair of HIP events on the launch
stream, nothing else running on the device; the median, the minimum and the maximum of the per-launch times are given.
A launch is the whole call: the plan, base and emit kernels in stream order. The parse of the same batch is timed the
same way in the same process. pcppx_sip_reference runs once on one core over the same batch and records, and the
device's output is compared with its output in every row. There is no earlier implementation to compare with: the file
holds what was measured.
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

from pcapplusplus_amd import abi, sip, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402
from pcapplusplus_amd.pcap import PacketBatch, from_packets  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
out_path = (sys.argv[3] if len(sys.argv) > 3 else None) or None

ML = 8
SHARES = (0.01, 1.0)
POOL = 4096
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)


def sip_packet(k: int) -> bytes:
    body = sip.sdp_body(f"10.{k % 200}.{k % 7}.{1 + k % 250}", 10000 + 2 * (k % 2000)) if k % 3 == 0 else b""
    h = sip.dialog_headers(k, body, bool(body))
    if k % 2 == 0:
        p = sip.request(abi.SIP_METHODS[k % 14], f"sip:user{k}@example.com", h, body)
    else:
        p = sip.response(sorted(sip.CODES)[k % 77], "Reason", h, body)
    if k % 5 == 0:
        return sip.packet(p, k, dport=6000 + k % 7)
    return sip.packet(p, k, tcp=k % 7 == 0)


def with_sip(b: PacketBatch, pool: PacketBatch, share: float) -> PacketBatch:
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


imix = synth.config(3, n)
pool = from_packets([sip_packet(k) for k in range(POOL)])
results = []
for share in SHARES:
    b = with_sip(imix, pool, share)
    data, offsets, caplens = to_device(b, dev)
    summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
    opts = abi.make_opts(0, 8, False, ML)
    parse = lambda: eng.parse_device(data, offsets, caplens, n, b.linktype, opts, summary, layers,  # noqa: E731
                                     st.cuda_stream)
    parse()
    p_ms = None
    for fields_mode, label in ((abi.HTTP_FIELDS_NONE, "NONE"), (abi.HTTP_FIELDS_WANTED, "WANTED")):
        spec = abi.make_sip_spec(abi.SIP_CALL_NAMES, fields_mode, 3)
        totals = torch.zeros(abi.SIP_TOTALS, dtype=torch.int64, device=dev)
        one = torch.empty(48, dtype=torch.uint8, device=dev)
        eng.sip_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, one, one, one, totals, 0, 0, 0,
                       stream=st.cuda_stream, summary=summary)
        torch.cuda.synchronize()
        need = abi.sip_totals_dict(totals.cpu().numpy().view(np.uint64))
        m, k, ns, nb = need["msgs"], need["fields"], need["sdps"], need["text_bytes"]
        msgs = torch.empty(max(m, 1) * 48, dtype=torch.uint8, device=dev)
        fields = torch.empty(max(k, 1) * 24, dtype=torch.uint8, device=dev)
        sdps = torch.empty(max(ns, 1) * 32, dtype=torch.uint8, device=dev)
        text = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
        disp = torch.empty(n, dtype=torch.uint8, device=dev)
        run = lambda: eng.sip_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, msgs, fields, sdps,  # noqa: E731
                                     totals, m, k, ns, text, nb, disp, st.cuda_stream, summary=summary)
        for _ in range(3):
            run()
            parse()
        torch.cuda.synchronize()
        tot = abi.sip_totals_dict(totals.cpu().numpy().view(np.uint64))
        assert tot["overflow"] == 0 and tot["msgs"] == m
        t_ms = per_launch(run, launches)
        p_ms = p_ms or per_launch(parse, launches)
        # the same batch and records through the host reference, one core
        h_sum, h_lay = summary.cpu().numpy(), layers.cpu().numpy()
        h_msgs, h_fields = np.empty(max(m, 1) * 48, np.uint8), np.empty(max(k, 1) * 24, np.uint8)
        h_sdps, h_text = np.empty(max(ns, 1) * 32, np.uint8), np.empty(nb + 64, np.uint8)
        h_disp, h_tot = np.empty(n, np.uint8), np.zeros(abi.SIP_TOTALS, np.uint64)
        hb = abi.Batch(b.data.ctypes.data, b.offsets.ctypes.data, b.caplens.ctypes.data, len(b.data), n, b.linktype, 0)
        ho = abi.SipOut(h_msgs.ctypes.data, h_fields.ctypes.data, h_sdps.ctypes.data, h_text.ctypes.data, nb,
                        h_disp.ctypes.data, m, k, ns, 0, h_tot.ctypes.data)
        t0 = time.perf_counter()
        abi.sip_reference(hb, abi.Records(h_sum.ctypes.data, h_lay.ctypes.data), ML, spec, ho)
        ref_ms = (time.perf_counter() - t0) * 1e3
        same = bool((msgs.cpu().numpy()[:m * 48] == h_msgs[:m * 48]).all() and
                    (fields.cpu().numpy()[:k * 24] == h_fields[:k * 24]).all() and
                    (sdps.cpu().numpy()[:ns * 32] == h_sdps[:ns * 32]).all() and
                    (text.cpu().numpy()[:nb] == h_text[:nb]).all() and (disp.cpu().numpy() == h_disp).all() and
                    list(totals.cpu().numpy().view(np.uint64)) == list(h_tot))
        med = statistics.median(t_ms)
        results.append({"sip_share": share, "fields": label, "packets": n, "messages": m, "requests": tot["requests"],
                        "responses": tot["responses"], "by_heuristic": tot["by_heuristic"], "sdps": ns, "records": k,
                        "text_bytes": nb, "header_bytes": tot["header_bytes"], "host_n": tot["host_n"],
                        "sip": stats(t_ms), "Mpps": round(n / med / 1e3, 1),
                        "messages_per_us": round(m / med / 1e3, 2),
                        "header_GB_per_s": round(tot["header_bytes"] / med / 1e6, 2), "parse": stats(p_ms),
                        "sip_over_parse": round(med / statistics.median(p_ms), 3),
                        "reference_one_core_ms": round(ref_ms, 2), "device_equals_reference": same})
        del msgs, fields, sdps, text, disp
    del data, offsets, caplens, summary, layers
    torch.cuda.empty_cache()
entry = {"kernel": "sip (plan + bases + emit)", "launches_per_case": launches, "warmup_launches": 3,
         "timing": "one HIP event pair per launch, median of the launches", "cases": results}
print(json.dumps(entry))
if out_path:
    p = Path(out_path)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(entry) + "\n")
eng.close()
assert all(r["device_equals_reference"] for r in results)
