"""Throughput of pcppx_defrag_device / pcppx_defrag6_device on a device-resident batch, against pcppx_select_device
keeping every packet.

  python tools/bench_defrag.py [packets] [launches] [percentages, e.g. 0,1,20] [--families 4|6|46[,...]] [--entry6]
                               [--base-lib path/to/an/older/libpcppx.so] [--device-input]

Workload: config-3 IMIX (10M packets by default) with 0 %, 1 % and 20 % of its IPv4 packets fragmented at 576 payload
bytes (pcapplusplus_amd.frag: IPFragUtil's rule), resident in HBM, parsed once with the reassembly front end
(pcppx_parse_batch_device_reasm: summary, layers, info). passthrough = 1: the output is IPDefragUtil's file, every
datagram whole. Two settings of max_fragments per case: 0 (= n: the table is sized, and cleared, for a batch of
nothing but fragments) and the power of two at or above the batch's candidates.
--families names what is timed, one variant per entry of a comma list: 4 (the default: the numbers stay comparable with
the earlier ones) is pcppx_defrag_device, and with --entry6 also pcppx_defrag6_device with families = V4; 6 and 46 are
pcppx_defrag6_device with families = V6 and V4 | V6. With a 6 or 46 in the list the same share of the batch's IPv6
packets is fragmented too (frag.fragment6, the ids the packet numbers; with --device-input by pcppx_frag6_device with
families = V6 over the same packets and ids instead, which gives the same batch without the host pass). --base-lib
adds pcppx_defrag_device of another build of the library (the parent commit's, say) as a variant, with a context of
its own in the same process.
Yardstick: pcppx_select_device with a keep-all mask over the same batch (it moves the same bytes but for the dropped
fragment headers), timed in the same process in rounds that alternate with the variants' launches, `launches` (>= 50)
launches of each between HIP events on the launch stream.
GB/s moved: 2 x OUT_BYTES over the time; ms_rounds: the per-launch time of every round (their spread is the noise
floor a comparison of two variants has to clear). Prints one JSON line.
"""
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, frag, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, frag6_on_device, parse_on_device, to_device  # noqa: E402


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
device_input = "--device-input" in argv
if device_input:
    argv.remove("--device-input")
families = option(argv, "--families", "4").split(",")
base_lib = option(argv, "--base-lib")
if not families or any(f not in ("4", "6", "46") for f in families):
    raise SystemExit("--families 4|6|46[,...]")
FAM_BITS = {"4": abi.DEFRAG_FAM_V4, "6": abi.DEFRAG_FAM_V6, "46": abi.DEFRAG_FAM_V4 | abi.DEFRAG_FAM_V6}
both = any(f != "4" for f in families)  # the batch's IPv6 packets are fragmented too
n0 = int(argv[0]) if len(argv) > 0 else 10_000_000
launches = max(int(argv[1]) if len(argv) > 1 else 50, 50)
pcts = [int(x) for x in argv[2].split(",")] if len(argv) > 2 else [0, 1, 20]
ROUNDS = 5
ML = 8
per_round = -(-launches // ROUNDS)
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)
base = synth.config(3, n0)
rng = np.random.default_rng(7)


def open_other(path: str) -> Engine:
    """pcppx_defrag_device of another build of the library, behind a context of its own."""
    lib = C.CDLL(str(Path(path).resolve()))
    lib.pcppx_open.restype = lib.pcppx_close.restype = lib.pcppx_defrag_device.restype = C.c_int
    lib.pcppx_defrag_device.argtypes = eng.lib.pcppx_defrag_device.argtypes
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
for pct in pcts:
    b = frag.fragment(base, 576, select=rng.random(base.n) < pct / 100) if pct else base
    if pct and both:  # a packet's fragments share its number, which is its fragment id
        chosen = (rng.random(base.n) < pct / 100)[b.meta["frag_src"]]
        if device_input:
            opts = abi.make_opts(0, 8, False, ML)
            b, *_ = frag6_on_device(eng, b, *parse_on_device(eng, b, opts), frag_size=576, families=abi.FRAG_FAM_V6,
                                    ids=b.meta["frag_src"], keep=chosen)
            b.data = np.concatenate([b.data, np.zeros(1, np.uint8)])
            torch.cuda.empty_cache()
        else:
            b = frag.fragment6(b, 576, b.meta["frag_src"], select=chosen)
    n = b.n
    print(f"{pct} % fragmented: {n} packets", file=sys.stderr, flush=True)
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
    is_fragment = status & 15 == abi.IPR_FRAGMENT
    fragments = int((is_fragment if both else is_fragment & (status & abi.IPR_F_IPV6 == 0)).sum())
    sized = 1 << max(int(fragments).bit_length(), 6)

    def variant(call, spec):
        return lambda: call(data, offsets, caplens, n, b.linktype, layers, ML, info, spec, out_off, out_cap, totals, n,
                            out_data, total, out_idx, out_first, out_frags, disp, st.cuda_stream, summary=summary)

    for max_fragments in (0, sized):
        old_spec = abi.make_defrag_spec(True, max_fragments)
        variants = []  # (name, launch)
        if base_eng is not None:
            variants.append(("base pcppx_defrag_device", variant(base_eng.defrag_device, old_spec)))
        for f in families:
            if f == "4":
                variants.append(("pcppx_defrag_device", variant(eng.defrag_device, old_spec)))
            if f != "4" or entry6:
                spec6 = abi.make_defrag6_spec(True, max_fragments, FAM_BITS[f])
                variants.append((f"pcppx_defrag6_device families={FAM_BITS[f]}", variant(eng.defrag6_device, spec6)))
        tots = []
        for _, run in variants:
            for _ in range(3):
                run()
                select()
            torch.cuda.synchronize()
            tot = abi.defrag_totals_dict(totals.cpu().numpy().view(np.uint64))
            assert tot["overflow"] == 0 and tot["candidates"] <= fragments
            if pct == 0 and tot["reassembled"] == 0:  # nothing to do: the output is the batch
                assert tot["out_bytes"] == total and bool(torch.equal(out_data[:total], data[:total]))
            tots.append(tot)
        rounds = [[] for _ in variants]
        s_rounds = []
        for _ in range(ROUNDS):
            for k, (_, run) in enumerate(variants):
                rounds[k].append(timed(run, per_round) / per_round)
            s_rounds.append(timed(select, per_round) / per_round)
        s_ms = sum(s_rounds) / ROUNDS
        print(f"{pct} % fragmented, max_fragments {max_fragments}: timed", file=sys.stderr, flush=True)
        for (name, _), tot, r in zip(variants, tots, rounds):
            d_ms = sum(r) / ROUNDS
            results.append({"variant": name, "fragmented_pct": pct, "packets": n, "batch_bytes": total,
                            "max_fragments": max_fragments, "candidates": tot["candidates"],
                            "reassembled": tot["reassembled"], "merged_frags": tot["merged_frags"],
                            "left_frags": tot["left_frags"], "out_packets": tot["out_packets"],
                            "out_bytes": tot["out_bytes"], "ms": round(d_ms, 4),
                            "GBps_moved": round(2 * tot["out_bytes"] / d_ms / 1e6, 1), "select_all_ms": round(s_ms, 4),
                            "select_GBps_moved": round(2 * total / s_ms / 1e6, 1),
                            "ratio_to_select": round(d_ms / s_ms, 2), "ms_rounds": [round(x, 4) for x in r],
                            "select_ms_rounds": [round(x, 4) for x in s_rounds]})
    del data, offsets, caplens, summary, layers, info, out_data, out_off, out_cap, out_idx, out_first, out_frags, disp
    torch.cuda.empty_cache()
print(json.dumps({"kernel": "defrag (collect + verdict + count + bases + place + merge + patch)",
                  "families": families, "ipv6_fragmented": both, "device_input": device_input, "base_lib": base_lib,
                  "source_packets": n0,
                  "frag_size": 576, "launches_per_case": ROUNDS * per_round, "cases": results}))
if base_eng is not None:
    base_eng.close()
eng.close()
