"""Throughput of pcppx_frag_device on a device-resident batch, against pcppx_select_device keeping every packet.

  python tools/bench_frag.py [packets] [launches] [out.json] [only]
      only: one case, e.g. 1500B:frag_size:576 or imix:mtu:576 (for a run under rocprofv3 --kernel-trace --stats)

Workloads: config-3 IMIX (64 / 512 / 1500 B at 7:4:1, 25 % VLAN, 30 % IPv6) and the same traffic at 1500 B only,
`packets` each (4M by default), resident in HBM and parsed once (summary, FIXED layers). Rules: frag_size 128, 576 and
1480 and mtu 576, every packet considered, copy_rest = 1 (IPFragUtil -a: the whole capture comes out). The output
buffers are sized by an index-only call, as a caller would.
Yardstick: pcppx_select_device with a keep-all mask over the same batch (a packed copy of the batch: the rate at which
this engine moves packets that it does not have to split), timed in the same process in rounds that alternate with the
frag launches, `launches` (>= 50) launches of each between HIP events on the launch stream.
GB/s moved: 2 x OUT_BYTES over the time (every output byte is read once and written once); for select 2 x the batch.
Prints one JSON line (and writes it to out.json when given).
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
out_path = (sys.argv[3] if len(sys.argv) > 3 else None) or None
only = sys.argv[4].split(":") if len(sys.argv) > 4 else None
ROUNDS = 5
ML = 8
RULES = (("frag_size", 128), ("frag_size", 576), ("frag_size", 1480), ("mtu", 576))
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


results = []
WORKLOADS = (("imix", lambda: synth.config(3, n)), ("1500B", lambda: synth.imix(n, 3, sizes=(1500,), weights=(1,))))
for workload, make in WORKLOADS:
    if only and only[0] != workload:
        continue
    b = make()
    total = int(b.caplens.sum(dtype=np.uint64))
    data, offsets, caplens = to_device(b, dev)
    summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
    eng.parse_device(data, offsets, caplens, n, b.linktype, abi.make_opts(0, 8, False, ML), summary, layers,
                     st.cuda_stream)
    totals = torch.zeros(abi.FRAG_TOTALS, dtype=torch.int64, device=dev)
    sel_totals = torch.zeros(abi.SEL_TOTALS, dtype=torch.int64, device=dev)
    sel_data = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    sel_off = torch.empty(n, dtype=torch.int64, device=dev)
    sel_cap = torch.empty(n, dtype=torch.int32, device=dev)
    sel_idx = torch.empty(n, dtype=torch.int32, device=dev)
    keep = torch.ones(n, dtype=torch.uint8, device=dev)
    sel_spec = abi.make_select_spec(keep=abi.ptr(keep))
    select = lambda: eng.select_device(data, offsets, caplens, n, b.linktype, sel_spec, sel_off, sel_cap,  # noqa: E731
                                       sel_totals, n, sel_data, total, sel_idx, st.cuda_stream)
    for mode, size in RULES:
        if only and (only[1], int(only[2])) != (mode, size):
            continue
        spec = abi.make_frag_spec(**{mode: size})
        one64, one32 = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        eng.frag_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, one64, one32, totals, 0,
                        stream=st.cuda_stream, summary=summary)  # the sizing call: index-only, no room
        torch.cuda.synchronize()
        need = abi.frag_totals_dict(totals.cpu().numpy().view(np.uint64))
        mp, cap = need["out_packets"], need["out_bytes"]
        out_data = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
        out_off = torch.empty(mp, dtype=torch.int64, device=dev)
        out_cap = torch.empty(mp, dtype=torch.int32, device=dev)
        out_idx = torch.empty(mp, dtype=torch.int32, device=dev)
        out_no = torch.empty(mp, dtype=torch.int16, device=dev)
        counts = torch.empty(n, dtype=torch.int16, device=dev)
        disp = torch.empty(n, dtype=torch.uint8, device=dev)
        run = lambda: eng.frag_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, out_off,  # noqa: E731
                                      out_cap, totals, mp, out_data, cap, out_idx, out_no, counts, disp, st.cuda_stream,
                                      summary=summary)
        for _ in range(3):
            run()
            select()
        torch.cuda.synchronize()
        tot = abi.frag_totals_dict(totals.cpu().numpy().view(np.uint64))
        assert tot["overflow"] == 0 and (tot["out_packets"], tot["out_bytes"]) == (mp, cap)
        f_ms = s_ms = 0.0
        for _ in range(ROUNDS):
            f_ms += timed(run, per_round)
            s_ms += timed(select, per_round)
        f_ms /= ROUNDS * per_round
        s_ms /= ROUNDS * per_round
        results.append({"workload": workload, mode: size, "packets": n, "batch_bytes": total,
                        "split_packets": tot["split_packets"], "fragments": tot["fragments"],
                        "out_packets": mp, "out_bytes": cap, "ms": round(f_ms, 4),
                        "GBps_moved": round(2 * cap / f_ms / 1e6, 1), "Mpps_out": round(mp / f_ms / 1e3, 1),
                        "select_all_ms": round(s_ms, 4), "select_GBps_moved": round(2 * total / s_ms / 1e6, 1),
                        "rate_vs_select": round((2 * cap / f_ms) / (2 * total / s_ms), 2)})
        del out_data, out_off, out_cap, out_idx, out_no, counts, disp
    del data, offsets, caplens, summary, layers, sel_data, sel_off, sel_cap, sel_idx, keep
    torch.cuda.empty_cache()
line = json.dumps({"kernel": "frag (plan + bases + emit + patch)", "source_packets": n,
                   "launches_per_case": ROUNDS * per_round, "cases": results})
print(line)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(line + "\n")
eng.close()
