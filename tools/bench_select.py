"""Throughput of pcppx_select_device on a device-resident batch, against a plain device-to-device copy.

  python tools/bench_select.py [packets] [launches]

Workload: config-3 IMIX (10M packets by default) resident in HBM, parsed once (its summary gives the flags case).
Cases: keep = all, random 1/2, random 1/64 (mask mode) and the batch's real PCPPX_F_NEEDS_HOST flags (flags mode,
stride 32); each with snaplen 0 and 96. Per case: warm-up, then `launches` (>= 50) select launches between HIP events
on the launch stream, in rounds that alternate with the yardstick -- a torch device-to-device copy of exactly
WRITTEN_BYTES bytes, timed the same way in the same process.
Algorithmic bytes of a select: the mask (1 B per source packet; flags mode 2 B) + 12 B of descriptors per source
packet + 2 x the bytes moved + 16 B (offset, caplen, index) per written packet. Prints one JSON line.
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
ROUNDS = 5
per_round = -(-launches // ROUNDS)

b = synth.config(3, n)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)
data, offsets, caplens = to_device(b, dev)
total = int(b.caplens.sum(dtype=np.uint64))
summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
eng.parse_device(data, offsets, caplens, n, b.linktype, abi.make_opts(0, 8, True, 0), summary, None, st.cuda_stream)
out_data = torch.empty(total + 64, dtype=torch.uint8, device=dev)
copy_dst = torch.empty(total + 64, dtype=torch.uint8, device=dev)
out_off = torch.empty(n, dtype=torch.int64, device=dev)
out_cap = torch.empty(n, dtype=torch.int32, device=dev)
out_idx = torch.empty(n, dtype=torch.int32, device=dev)
totals = torch.zeros(abi.SEL_TOTALS, dtype=torch.int64, device=dev)
rng = np.random.default_rng(12)
masks = {"all": np.ones(n, np.uint8), "half": (rng.random(n) < 0.5).astype(np.uint8),
         "1in64": (rng.random(n) < 1 / 64).astype(np.uint8)}
masks_t = {k: torch.from_numpy(v).to(dev) for k, v in masks.items()}


def spec_for(case: str, snaplen: int) -> abi.SelectSpec:
    if case == "needs_host":
        return abi.make_select_spec(flags=abi.ptr(summary) + abi.FLAGS_OFFSET, flags_stride=32,
                                    flags_any=abi.F_NEEDS_HOST, snaplen=snaplen)
    return abi.make_select_spec(keep=abi.ptr(masks_t[case]), snaplen=snaplen)


def timed(fn, reps: int) -> float:
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    z.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(z)


results = []
for case in ("all", "half", "1in64", "needs_host"):
    for snaplen in (0, 96):
        spec = spec_for(case, snaplen)
        run = lambda: eng.select_device(data, offsets, caplens, n, b.linktype, spec, out_off, out_cap, totals, n,  # noqa: E731
                                        out_data, total, out_idx, st.cuda_stream)
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        tot = abi.totals_dict(totals.cpu().numpy().view(np.uint64))
        wb, wp = tot["written_bytes"], tot["written_packets"]
        if case == "all" and snaplen == 0:  # keep-everything over a packed batch reproduces it: checked at full size
            assert wb == total and wp == n and bool(torch.equal(out_data[:total], data[:total]))
            assert bool(torch.equal(out_off, offsets)) and bool(torch.equal(out_cap, caplens))
        src_v, dst_v = data[:wb], copy_dst[:wb]
        copy = lambda: dst_v.copy_(src_v)  # noqa: E731
        for _ in range(3):
            copy()
        sel_ms = cp_ms = 0.0
        for _ in range(ROUNDS):
            sel_ms += timed(run, per_round)
            cp_ms += timed(copy, per_round)
        sel_ms /= ROUNDS * per_round
        cp_ms /= ROUNDS * per_round
        algo = (2 if case == "needs_host" else 1) * n + 12 * n + 2 * wb + 16 * wp
        results.append({"keep": case, "snaplen": snaplen, "written_packets": wp, "written_bytes": wb,
                        "ms": round(sel_ms, 4), "algorithmic_bytes": algo, "GBps": round(algo / sel_ms / 1e6, 1),
                        "copy_ms": round(cp_ms, 4), "copy_GBps": round(2 * wb / cp_ms / 1e6, 1) if wb else 0.0,
                        "ratio_to_copy": round(sel_ms / cp_ms, 2) if wb else None})
print(json.dumps({"kernel": "select (count + base + copy)", "packets": n, "batch_bytes": total,
                  "launches_per_case": ROUNDS * per_round, "cases": results}))
eng.close()
