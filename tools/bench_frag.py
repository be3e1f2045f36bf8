"""Throughput of pcppx_frag_device / pcppx_frag6_device on a device-resident batch, against pcppx_select_device keeping
every packet.

  python tools/bench_frag.py [packets] [launches] [out.json] [only] [--families 4|6|46[,...]] [--entry6]
                             [--base-lib path/to/an/older/libpcppx.so]
      only: one case, e.g. 1500B:frag_size:576 or imix:mtu:576 (for a run under rocprofv3 --kernel-trace --stats)
      --families: what is timed, one variant per entry of a comma list. 4 (the default: the numbers stay comparable
          with the earlier ones) is pcppx_frag_device, and with --entry6 also pcppx_frag6_device with families = V4;
          6 and 46 are pcppx_frag6_device with families = V6 and V4 | V6 (ids: id_base 0). The variants of a case run
          over the same batch in rounds that alternate; each sizes its own output.
      --base-lib: adds pcppx_frag_device of another build of the library (the parent commit's, say) as a variant,
          with a context of its own in the same process.

Workloads: config-3 IMIX (64 / 512 / 1500 B at 7:4:1, 25 % VLAN, 30 % IPv6) and the same traffic at 1500 B only,
`packets` each (4M by default), resident in HBM and parsed once (summary, FIXED layers). Rules: frag_size 128, 576 and
1480 and mtu 576, every packet considered, copy_rest = 1 (IPFragUtil -a: the whole capture comes out). The output
buffers are sized by an index-only call, as a caller would.
Yardstick: pcppx_select_device with a keep-all mask over the same batch (a packed copy of the batch: the rate at which
this engine moves packets that it does not have to split), timed in the same process in rounds that alternate with the
frag launches, `launches` (>= 50) launches of each between HIP events on the launch stream.
GB/s moved: 2 x OUT_BYTES over the time (every output byte is read once and written once); for select 2 x the batch.
ms_rounds: the per-launch time of every round (their spread is the noise floor a comparison of two variants has to
clear). Prints one JSON line (and writes it to out.json when given).
"""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402


def option(argv: list, name: str, default=None):
    if name not in argv:
        return default
    k = argv.index(name)
    value = argv[k + 1]
    del argv[k:k + 2]
    return value


argv = list(sys.argv[1:])
entry6 = "--entry6" in argv
if entry6:
    argv.remove("--entry6")
families = option(argv, "--families", "4").split(",")
base_lib = option(argv, "--base-lib")
if not families or any(f not in ("4", "6", "46") for f in families):
    raise SystemExit("--families 4|6|46[,...]")
FAM_BITS = {"4": abi.FRAG_FAM_V4, "6": abi.FRAG_FAM_V6, "46": abi.FRAG_FAM_V4 | abi.FRAG_FAM_V6}
n = int(argv[0]) if len(argv) > 0 else 4_000_000
launches = max(int(argv[1]) if len(argv) > 1 else 50, 50)
out_path = (argv[2] if len(argv) > 2 else None) or None
only = argv[3].split(":") if len(argv) > 3 else None
ROUNDS = 5
ML = 8
RULES = (("frag_size", 128), ("frag_size", 576), ("frag_size", 1480), ("mtu", 576))
per_round = -(-launches // ROUNDS)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)


def open_other(path: str) -> Engine:
    """pcppx_frag_device of another build of the library, behind a context of its own."""
    lib = C.CDLL(str(Path(path).resolve()))
    lib.pcppx_open.restype = lib.pcppx_close.restype = lib.pcppx_frag_device.restype = C.c_int
    lib.pcppx_frag_device.argtypes = eng.lib.pcppx_frag_device.argtypes
    other = Engine.__new__(Engine)
    other.lib, other.ctx, other.device = lib, C.c_void_p(), 0
    abi.check(lib.pcppx_open(0, C.byref(other.ctx)), "pcppx_open (base library)")
    return other


base_eng = open_other(base_lib) if base_lib else None


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
        old_spec = abi.make_frag_spec(**{mode: size})
        named = []  # (name, call, spec)
        if base_eng is not None:
            named.append(("base pcppx_frag_device", base_eng.frag_device, old_spec))
        for f in families:
            if f == "4":
                named.append(("pcppx_frag_device", eng.frag_device, old_spec))
            if f != "4" or entry6:
                named.append((f"pcppx_frag6_device families={FAM_BITS[f]}", eng.frag6_device,
                              abi.make_frag6_spec(families=FAM_BITS[f], **{mode: size})))
        one64, one32 = torch.empty(1, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        variants = []  # (name, launch, the totals of its sizing call, its buffers)
        for name, call, spec in named:
            call(data, offsets, caplens, n, b.linktype, layers, ML, spec, one64, one32, totals, 0,
                 stream=st.cuda_stream, summary=summary)  # the sizing call: index-only, no room
            torch.cuda.synchronize()
            need = abi.frag_totals_dict(totals.cpu().numpy().view(np.uint64))
            mp, cap = need["out_packets"], need["out_bytes"]
            bufs = (torch.empty(mp, dtype=torch.int64, device=dev), torch.empty(mp, dtype=torch.int32, device=dev),
                    torch.empty(cap + 64, dtype=torch.uint8, device=dev),
                    torch.empty(mp, dtype=torch.int32, device=dev),
                    torch.empty(mp, dtype=torch.int16, device=dev), torch.empty(n, dtype=torch.int16, device=dev),
                    torch.empty(n, dtype=torch.uint8, device=dev))

            def run(call=call, spec=spec, mp=mp, cap=cap, bufs=bufs):
                out_off, out_cap, out_data, out_idx, out_no, counts, disp = bufs
                call(data, offsets, caplens, n, b.linktype, layers, ML, spec, out_off, out_cap, totals, mp, out_data,
                     cap, out_idx, out_no, counts, disp, st.cuda_stream, summary=summary)

            for _ in range(3):
                run()
                select()
            torch.cuda.synchronize()
            tot = abi.frag_totals_dict(totals.cpu().numpy().view(np.uint64))
            assert tot["overflow"] == 0 and (tot["out_packets"], tot["out_bytes"]) == (mp, cap)
            variants.append((name, run, tot, bufs))
        rounds = [[] for _ in variants]
        s_rounds = []
        for _ in range(ROUNDS):
            for k, (_, run, _, _) in enumerate(variants):
                rounds[k].append(timed(run, per_round) / per_round)
            s_rounds.append(timed(select, per_round) / per_round)
        s_ms = sum(s_rounds) / ROUNDS
        for (name, _, tot, _), r in zip(variants, rounds):
            f_ms = sum(r) / ROUNDS
            mp, cap = tot["out_packets"], tot["out_bytes"]
            results.append({"variant": name, "workload": workload, mode: size, "packets": n, "batch_bytes": total,
                            "split_packets": tot["split_packets"], "fragments": tot["fragments"],
                            "out_packets": mp, "out_bytes": cap, "ms": round(f_ms, 4),
                            "GBps_moved": round(2 * cap / f_ms / 1e6, 1), "Mpps_out": round(mp / f_ms / 1e3, 1),
                            "select_all_ms": round(s_ms, 4), "select_GBps_moved": round(2 * total / s_ms / 1e6, 1),
                            "rate_vs_select": round((2 * cap / f_ms) / (2 * total / s_ms), 2),
                            "ratio_to_select": round(f_ms / s_ms, 2), "ms_rounds": [round(x, 4) for x in r],
                            "select_ms_rounds": [round(x, 4) for x in s_rounds]})
        del variants
    del data, offsets, caplens, summary, layers, sel_data, sel_off, sel_cap, sel_idx, keep
    torch.cuda.empty_cache()
line = json.dumps({"kernel": "frag (plan + bases + emit + patch)", "families": families, "base_lib": base_lib,
                   "source_packets": n,
                   "launches_per_case": ROUNDS * per_round, "cases": results})
print(line)
if out_path:
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    Path(out_path).write_text(line + "\n")
if base_eng is not None:
    base_eng.close()
eng.close()
