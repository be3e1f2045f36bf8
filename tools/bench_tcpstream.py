"""Throughput of pcppx_tcpstream_device on a device-resident batch, against pcppx_select_device keeping every packet.

  python tools/bench_tcpstream.py [packets] [launches] [flows]

Workload: a config-4-like batch (pcapplusplus_amd.tcpstream.session_batch): one stream of Ethernet + IPv4 + TCP packets
with payload, IMIX sizes, their connections drawn from `flows` (1M by default) with a Zipf law, so that a few elephant
sides have thousands of segments and most sides a few; every side continues its sequence numbers in arrival order, so
all of them are reassembled (but for the few flows whose 32-bit hash5 collide: one connection with a third source).
Resident in HBM, parsed once with the reassembly front end (pcppx_parse_batch_device_reasm: summary, layers, info).
Yardstick: pcppx_select_device with a keep-all mask over the same batch, the existing mover nearest in work (it moves
the packets whole, tcpstream their payloads only), timed in the same process in rounds that alternate with the
tcpstream launches, `launches` (>= 50) launches of each between HIP events on the launch stream, after 3 warm-up
launches. Payload GB/s: 2 x BYTES (read + written) over the time. Prints one JSON line.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, tcpstream  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
flows = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
ROUNDS = 5
ML = 8
per_round = -(-launches // ROUNDS)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)


def timed(fn, reps: int) -> float:
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    z.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(z)


b, side = tcpstream.session_batch(n, flows)
total = int(b.caplens.sum(dtype=np.uint64))
per_side = np.bincount(np.unique(side, return_inverse=True)[1])
data, offsets, caplens = to_device(b, dev)
summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
info = torch.empty(n * 16, dtype=torch.uint8, device=dev)
eng.parse_reasm_device(data, offsets, caplens, n, b.linktype, abi.make_opts(0, 8, False, ML), summary, layers, info,
                       st.cuda_stream)
out_data = torch.empty(total + 64, dtype=torch.uint8, device=dev)
streams = torch.empty(n * abi.TCPSTREAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
disp = torch.empty(n, dtype=torch.uint8, device=dev)
seg_stream = torch.empty(n, dtype=torch.int32, device=dev)
seg_pos = torch.empty(n, dtype=torch.int32, device=dev)
totals = torch.zeros(abi.TCPS_TOTALS, dtype=torch.int64, device=dev)
out_off = torch.empty(n, dtype=torch.int64, device=dev)
out_cap = torch.empty(n, dtype=torch.int32, device=dev)
out_idx = torch.empty(n, dtype=torch.int32, device=dev)
sel_totals = torch.zeros(abi.SEL_TOTALS, dtype=torch.int64, device=dev)
keep = torch.ones(n, dtype=torch.uint8, device=dev)
sel_spec = abi.make_select_spec(keep=abi.ptr(keep))
select = lambda: eng.select_device(data, offsets, caplens, n, b.linktype, sel_spec, out_off, out_cap,  # noqa: E731
                                   sel_totals, n, out_data, total, out_idx, st.cuda_stream)
spec = abi.make_tcpstream_spec(True, 0)
results = []
for what, with_data in (("streams", True), ("index_only", False)):
    run = lambda: eng.tcpstream_device(data, offsets, caplens, n, b.linktype, layers, ML, info, spec,  # noqa: E731
                                       streams, totals, n, out_data if with_data else None, total, disp, seg_stream,
                                       seg_pos, st.cuda_stream, summary=summary)
    for _ in range(3):
        run()
        select()
    torch.cuda.synchronize()
    tot = abi.tcpstream_totals_dict(totals.cpu().numpy().view(np.uint64))
    # flows whose 32-bit hash5 collide are one connection with more than two sources: their later packets are LEFT
    assert tot["overflow"] == 0 and tot["candidates"] == n and tot["segments"] + tot["left"] == n, tot
    assert tot["left"] <= n // 1000, tot
    t_ms = s_ms = 0.0
    for _ in range(ROUNDS):
        t_ms += timed(run, per_round)
        s_ms += timed(select, per_round)
    t_ms /= ROUNDS * per_round
    s_ms /= ROUNDS * per_round
    results.append({"mode": what, "streams": tot["streams"], "segments": tot["segments"], "left": tot["left"],
                    "payload_bytes": tot["bytes"], "ms": round(t_ms, 4),
                    "payload_GBps": round(2 * tot["bytes"] / t_ms / 1e6, 1) if with_data else None,
                    "Mpps": round(n / t_ms / 1e3, 1), "select_all_ms": round(s_ms, 4),
                    "select_GBps_moved": round(2 * total / s_ms / 1e6, 1), "ratio_to_select": round(t_ms / s_ms, 2)})
print(json.dumps({"kernel": "tcpstream (2 clears + collect, second, join, chain, verdict, count, bases, place, emit)",
                  "packets": n, "flows": flows, "batch_bytes": total, "sides": int(len(per_side)),
                  "largest_side_segments": int(per_side.max()), "launches_per_case": ROUNDS * per_round,
                  "device": abi.runtime_info(0), "cases": results}))
eng.close()
