"""Throughput of pcppx_defrag_device on a device-resident batch, against pcppx_select_device keeping every packet.

  python tools/bench_defrag.py [packets] [launches] [percentages, e.g. 0,1,20]

Workload: config-3 IMIX (10M packets by default) with 0 %, 1 % and 20 % of its IPv4 packets fragmented at 576 payload
bytes (pcapplusplus_amd.frag: IPFragUtil's rule), resident in HBM, parsed once with the reassembly front end
(pcppx_parse_batch_device_reasm: summary, layers, info). passthrough = 1: the output is IPDefragUtil's file, every
datagram whole. Two settings of max_fragments per case: 0 (= n: the table is sized, and cleared, for a batch of
nothing but fragments) and the power of two at or above the batch's candidates.
Yardstick: pcppx_select_device with a keep-all mask over the same batch (it moves the same bytes but for the dropped
fragment headers), timed in the same process in rounds that alternate with the defrag launches, `launches` (>= 50)
launches of each between HIP events on the launch stream.
GB/s moved: 2 x OUT_BYTES over the time. Prints one JSON line.
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, frag, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402

n0 = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
pcts = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else [0, 1, 20]
ROUNDS = 5
ML = 8
per_round = -(-launches // ROUNDS)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)
base = synth.config(3, n0)
rng = np.random.default_rng(7)


def timed(fn, reps: int) -> float:
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    for _ in range(reps):
        fn()
    z.record(st)
    torch.cuda.synchronize()
    return a.elapsed_time(z)


results = []
for pct in pcts:
    b = frag.fragment(base, 576, select=rng.random(base.n) < pct / 100) if pct else base
    n = b.n
    total = int(b.caplens.sum(dtype=np.uint64))
    data, offsets, caplens = to_device(b, dev)
    summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
    info = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    eng.parse_reasm_device(data, offsets, caplens, n, b.linktype, abi.make_opts(0, 8, False, ML), summary, layers, info,
                           st.cuda_stream)
    out_data = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    out_off = torch.empty(n, dtype=torch.int64, device=dev)
    out_cap = torch.empty(n, dtype=torch.int32, device=dev)
    out_idx = torch.empty(n, dtype=torch.int32, device=dev)
    out_first = torch.empty(n, dtype=torch.int32, device=dev)
    out_frags = torch.empty(n, dtype=torch.uint8, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    totals = torch.zeros(abi.DEFRAG_TOTALS, dtype=torch.int64, device=dev)
    sel_totals = torch.zeros(abi.SEL_TOTALS, dtype=torch.int64, device=dev)
    keep = torch.ones(n, dtype=torch.uint8, device=dev)
    sel_spec = abi.make_select_spec(keep=abi.ptr(keep))
    select = lambda: eng.select_device(data, offsets, caplens, n, b.linktype, sel_spec, out_off, out_cap,  # noqa: E731
                                       sel_totals, n, out_data, total, out_idx, st.cuda_stream)
    torch.cuda.synchronize()
    status = info.cpu().numpy().view(abi.REASM_DTYPE)["ip_status"]
    fragments = int(((status & 15 == abi.IPR_FRAGMENT) & (status & abi.IPR_F_IPV6 == 0)).sum())
    sized = 1 << max(int(fragments).bit_length(), 6)
    for max_fragments in (0, sized):
        spec = abi.make_defrag_spec(True, max_fragments)
        run = lambda: eng.defrag_device(data, offsets, caplens, n, b.linktype, layers, ML, info, spec,  # noqa: E731
                                        out_off, out_cap, totals, n, out_data, total, out_idx, out_first, out_frags,
                                        disp, st.cuda_stream, summary=summary)
        for _ in range(3):
            run()
            select()
        torch.cuda.synchronize()
        tot = abi.defrag_totals_dict(totals.cpu().numpy().view(np.uint64))
        assert tot["overflow"] == 0 and tot["candidates"] <= fragments
        if pct == 0 and tot["reassembled"] == 0:  # nothing to do: the output is the batch
            assert tot["out_bytes"] == total and bool(torch.equal(out_data[:total], data[:total]))
        d_ms = s_ms = 0.0
        for _ in range(ROUNDS):
            d_ms += timed(run, per_round)
            s_ms += timed(select, per_round)
        d_ms /= ROUNDS * per_round
        s_ms /= ROUNDS * per_round
        results.append({"fragmented_pct": pct, "packets": n, "batch_bytes": total, "max_fragments": max_fragments,
                        "candidates": tot["candidates"], "reassembled": tot["reassembled"],
                        "merged_frags": tot["merged_frags"], "left_frags": tot["left_frags"],
                        "out_packets": tot["out_packets"], "out_bytes": tot["out_bytes"], "ms": round(d_ms, 4),
                        "GBps_moved": round(2 * tot["out_bytes"] / d_ms / 1e6, 1), "select_all_ms": round(s_ms, 4),
                        "select_GBps_moved": round(2 * total / s_ms / 1e6, 1), "ratio_to_select": round(d_ms / s_ms, 2)})
    del data, offsets, caplens, summary, layers, info, out_data, out_off, out_cap, out_idx, out_first, out_frags, disp
    torch.cuda.empty_cache()
print(json.dumps({"kernel": "defrag (collect + verdict + count + bases + place + merge + patch)", "source_packets": n0,
                  "frag_size": 576, "launches_per_case": ROUNDS * per_round, "cases": results}))
eng.close()
