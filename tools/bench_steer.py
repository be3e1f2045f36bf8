"""Time of pcppx_steer_device on a device-resident batch, against a plain device-to-device copy of the same bytes and
against pcppx_select_device keep-everything.

  python tools/bench_steer.py [--packets N] [--launches L] [--out profiles/steer_bench.json] [--no-check]

Workload: config-3 IMIX (10M packets by default) resident in HBM, parsed once on the device; its summary's hash5 column
is the key (stride 32). Configurations: key mode with K = 1, 8, 64, 256, and one column-mode run (K = 8, the bucket
column = hash5 % 8 computed on the host, so it moves the same packets to the same places). Per configuration: warm-up,
then `launches` (>= 20) launches, each between its own pair of HIP events on the launch stream; the median is reported
(min and max beside it). The two yardsticks are timed the same way in the same process: a torch device-to-device copy
of exactly the batch's bytes, and pcppx_select_device with a keep-everything mask.
Every configuration's output is compared once, at full size, with pcppx_steer_reference (data, offsets, caplens, index,
bucket_first, bucket_pos, totals): this is where the deepest steps of the scan kernels are certain to run.
Algorithmic bytes of a steer: the key (4 B; column mode 1 B) + 12 B of descriptors per source packet + 2 x the bytes
moved + 16 B (offset, caplen, index) per steered packet. Writes one JSON document to --out and prints it.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=10_000_000)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--out", default=str(ROOT / "profiles" / "steer_bench.json"))
ap.add_argument("--no-check", action="store_true", help="skip the full-size comparison with pcppx_steer_reference")
ap.add_argument("--only", default="", help="one configuration, e.g. key8 (for a kernel trace run)")
args = ap.parse_args()
n, launches = args.packets, max(args.launches, 20)

b = synth.config(3, n)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)
data, offsets, caplens = to_device(b, dev)
total = int(b.caplens.sum(dtype=np.uint64))
summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
eng.parse_device(data, offsets, caplens, n, b.linktype, abi.make_opts(0, 8, True, 0), summary, None, st.cuda_stream)
torch.cuda.synchronize()
H5 = abi.SUMMARY_DTYPE.fields["hash5"][1]
hash5 = np.ascontiguousarray(summary.cpu().numpy().view(abi.SUMMARY_DTYPE)["hash5"])
out_data = torch.empty(total + 64, dtype=torch.uint8, device=dev)
copy_dst = torch.empty(total + 64, dtype=torch.uint8, device=dev)
out_off = torch.empty(n, dtype=torch.int64, device=dev)
out_cap = torch.empty(n, dtype=torch.int32, device=dev)
out_idx = torch.empty(n, dtype=torch.int32, device=dev)
first = torch.empty(abi.STEER_MAX_BUCKETS + 1, dtype=torch.int32, device=dev)
pos = torch.empty(abi.STEER_MAX_BUCKETS + 1, dtype=torch.int64, device=dev)
totals = torch.zeros(abi.STEER_TOTALS, dtype=torch.int64, device=dev)
keep_all = torch.ones(n, dtype=torch.uint8, device=dev)


def timed(fn) -> dict:
    """Warm-up, then `launches` launches, each between its own events: median / min / max in ms."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, z in ev:
        a.record(st)
        fn()
        z.record(st)
    torch.cuda.synchronize()
    ms = [a.elapsed_time(z) for a, z in ev]
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def check(K: int, col) -> None:
    """The device output of the last launch against pcppx_steer_reference, every array, at full size."""
    r_data = np.empty(total + 64, np.uint8)
    r_off, r_cap, r_idx = np.empty(n, np.uint64), np.empty(n, np.uint32), np.empty(n, np.uint32)
    r_first, r_pos, r_tot = np.empty(K + 1, np.uint32), np.empty(K + 1, np.uint64), np.empty(abi.STEER_TOTALS, np.uint64)
    rb = abi.Batch(b.data.ctypes.data, b.offsets.ctypes.data, b.caplens.ctypes.data, int(b.data.nbytes), n, b.linktype, 0)
    spec = (abi.make_steer_spec(bucket=col.ctypes.data, n_buckets=K) if col is not None
            else abi.make_steer_spec(key=hash5.ctypes.data, key_stride=4, n_buckets=K))
    ro = abi.Steering(r_data.ctypes.data, total, r_off.ctypes.data, r_cap.ctypes.data, r_idx.ctypes.data,
                      r_first.ctypes.data, r_pos.ctypes.data, n, 0, r_tot.ctypes.data)
    abi.steer_reference(rb, spec, ro)
    got = totals.cpu().numpy().view(np.uint64)
    assert list(got) == list(r_tot) and int(r_tot[abi.STEER_OVERFLOW]) == 0, (K, list(got), list(r_tot))
    assert int(r_tot[abi.STEER_STEERED_PACKETS]) == n and int(r_tot[abi.STEER_STEERED_BYTES]) == total
    assert np.array_equal(first[:K + 1].cpu().numpy().view(np.uint32), r_first), K
    assert np.array_equal(pos[:K + 1].cpu().numpy().view(np.uint64), r_pos), K
    assert np.array_equal(out_idx.cpu().numpy().view(np.uint32), r_idx), K
    assert np.array_equal(out_off.cpu().numpy().view(np.uint64), r_off), K
    assert np.array_equal(out_cap.cpu().numpy().view(np.uint32), r_cap), K
    assert np.array_equal(out_data[:total].cpu().numpy(), r_data[:total]), K


src_v, dst_v = data[:total], copy_dst[:total]
copy = timed(lambda: dst_v.copy_(src_v))
copy["GBps"] = round(2 * total / copy["ms"] / 1e6, 1)
sel_spec = abi.make_select_spec(keep=abi.ptr(keep_all))
sel = timed(lambda: eng.select_device(data, offsets, caplens, n, b.linktype, sel_spec, out_off, out_cap, totals, n,
                                      out_data, total, out_idx, st.cuda_stream))
sel["ratio_to_copy"] = round(sel["ms"] / copy["ms"], 2)

configs = [("key", 1), ("key", 8), ("key", 64), ("key", 256), ("column", 8)]
results = []
for mode, K in configs:
    if args.only and args.only != f"{mode}{K}":
        continue
    col = (hash5 % np.uint32(K)).astype(np.uint8) if mode == "column" else None
    col_t = torch.from_numpy(col).to(dev) if col is not None else None
    spec = (abi.make_steer_spec(bucket=abi.ptr(col_t), n_buckets=K) if col is not None
            else abi.make_steer_spec(key=abi.ptr(summary) + H5, key_stride=32, n_buckets=K))
    run = lambda: eng.steer_device(data, offsets, caplens, n, b.linktype, spec, out_off, out_cap, first, pos,  # noqa: E731
                                   totals, n, out_data, total, out_idx, st.cuda_stream)
    t = timed(run)
    if not args.no_check:
        check(K, col)
    algo = (1 if col is not None else 4) * n + 12 * n + 2 * total + 16 * n
    t.update({"mode": mode, "n_buckets": K, "algorithmic_bytes": algo, "GBps": round(algo / t["ms"] / 1e6, 1),
              "ratio_to_copy": round(t["ms"] / copy["ms"], 2), "ratio_to_select_all": round(t["ms"] / sel["ms"], 2),
              "checked_against_reference": not args.no_check})
    results.append(t)
doc = {"kernel": "steer (count + scan + bases + copy)", "packets": n, "batch_bytes": total, "launches_per_case": launches,
       "statistic": "median of per-launch HIP event times", "copy": copy, "select_keep_everything": sel, "cases": results}
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(doc) + "\n")
print(json.dumps(doc))
eng.close()
