"""Time of pcppx_bpf_device on a device-resident batch, against the parse-only SHORT launch that writes tuples for the
same batch.

  python tools/bench_bpf.py [--packets N] [--launches L] [--runs R] [--out profiles/bpf_bench.json] [--no-check]
                            [--only NAME]

Workload: config-3 IMIX (10M packets by default) resident in HBM. Four filters:
  ret1         `ret #1`: the descriptor reads, the verdict writes and the launch -- the floor
  tcp_port     "IPv4, not a later fragment, TCP, dst port P" over untagged Ethernet (11 instructions, bpf.tcp_dst_port)
  ip_ip6_port  TCP or UDP to dst port P over IPv4 (no later fragment, any header length) or IPv6, VLAN-tagged frames
               rejected: 30 instructions with an IPv4 and an IPv6 branch
  classify16   16 programs as a classifier: program q accepts TCP / UDP over IPv4 whose dst port has (port & 15) == q
The yardstick, timed the same way in the same process: the parse-only launch (no checksums, no layers, the SHORT
window) that writes the 48-B tuples of the same batch. It reads the same header lines and does more work per packet, so
it is what a filter that looks only at headers is measured against.
Per case and run: warm-up, then `launches` (>= 20) launches, each between its own pair of HIP events on the launch
stream, the median taken; `runs` (>= 3) such runs, and the median, lowest and highest of the runs' medians reported.
Every filter's full-size output is checked: the device's matched / bucket / ret of a seeded sample of the packets
against pcppx_bpf_reference over the same descriptors, totals[MATCHED] against the whole matched column, and the totals
against the reference's over the whole batch. P defaults to a port that occurs in the batch.
Writes one JSON document to --out and prints it.
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

from pcapplusplus_amd import abi, bpf, synth  # noqa: E402
from pcapplusplus_amd.bpf import (ABS, ALU, AND, IND, JEQ, JMP, JSET, LD, LDX, MSH, RET, B, H, K, insn)  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--packets", type=int, default=10_000_000)
ap.add_argument("--launches", type=int, default=30)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--sample", type=int, default=1_000_000)
ap.add_argument("--port", type=int, default=0, help="0: the dst port of the batch's first plain IPv4 / TCP packet")
ap.add_argument("--out", default=str(ROOT / "profiles" / "bpf_bench.json"))
ap.add_argument("--no-check", action="store_true", help="skip the comparison with pcppx_bpf_reference")
ap.add_argument("--only", default="", help="one case, e.g. tcp_port (for a kernel trace run)")
args = ap.parse_args()
n, launches, runs, PORT = args.packets, max(args.launches, 20), max(args.runs, 3), args.port
b = synth.config(3, n)
if PORT == 0:  # the synthetic ports are random: take one that occurs
    for i in range(b.n):
        pk = b.data[int(b.offsets[i]): int(b.offsets[i]) + 38]
        if len(pk) == 38 and pk[12] == 8 and pk[13] == 0 and pk[14] == 0x45 and pk[23] == 6:
            PORT = int(pk[36]) << 8 | int(pk[37])
            break


def ip_ip6_port(port: int) -> np.ndarray:
    """TCP or UDP to dst port `port`, over IPv4 (not a later fragment) or IPv6 (no extension headers)."""
    return bpf.program([
        insn(LD | H | ABS, k=12),                   # 0
        insn(JMP | JEQ | K, 0, 10, 0x0800),         # 1  not IPv4 -> 12
        insn(LD | B | ABS, k=23),                   # 2
        insn(JMP | JEQ | K, 1, 0, 6),               # 3  TCP -> 5
        insn(JMP | JEQ | K, 0, 24, 17),             # 4  not UDP -> 29
        insn(LD | H | ABS, k=20),                   # 5
        insn(JMP | JSET | K, 22, 0, 0x1FFF),        # 6  a later fragment -> 29
        insn(LDX | B | MSH, k=14),                  # 7
        insn(LD | H | IND, k=16),                   # 8
        insn(JMP | JEQ | K, 18, 19, port),          # 9  -> 28 / 29
        insn(RET | K, k=0),                         # 10 (not reached: keeps the branches apart)
        insn(RET | K, k=0),                         # 11
        insn(JMP | JEQ | K, 0, 16, 0x86DD),         # 12 not IPv6 -> 29
        insn(LD | B | ABS, k=20),                   # 13 next header
        insn(JMP | JEQ | K, 1, 0, 6),               # 14 TCP -> 16
        insn(JMP | JEQ | K, 0, 13, 17),             # 15 not UDP -> 29
        insn(LD | B | ABS, k=14),                   # 16 version nibble
        insn(ALU | AND | K, k=0xF0),                # 17
        insn(JMP | JEQ | K, 0, 10, 0x60),           # 18 -> 29
        insn(LD | H | ABS, k=18),                   # 19 payload length
        insn(JMP | bpf.JGE | K, 0, 8, 4),           # 20 room for the ports, else -> 29
        insn(LD | H | ABS, k=56),                   # 21 dst port
        insn(JMP | JEQ | K, 5, 0, port),            # 22 -> 28
        insn(LD | H | ABS, k=54),                   # 23 src port: the reverse direction as well
        insn(JMP | JEQ | K, 0, 4, port),            # 24 -> 29
        insn(LD | B | ABS, k=21),                   # 25 hop limit
        insn(JMP | bpf.JGT | K, 1, 2, 0),           # 26 -> 28 / 29
        insn(RET | K, k=0),                         # 27
        insn(RET | K, k=262144),                    # 28
        insn(RET | K, k=0),                         # 29
    ])


def classify(q: int) -> np.ndarray:
    """Program q of 16: TCP / UDP over IPv4, not a later fragment, (dst port & 15) == q."""
    return bpf.program([
        insn(LD | H | ABS, k=12), insn(JMP | JEQ | K, 0, 10, 0x0800), insn(LD | B | ABS, k=23),
        insn(JMP | JEQ | K, 1, 0, 6), insn(JMP | JEQ | K, 0, 7, 17), insn(LD | H | ABS, k=20),
        insn(JMP | JSET | K, 5, 0, 0x1FFF), insn(LDX | B | MSH, k=14), insn(LD | H | IND, k=16),
        insn(ALU | AND | K, k=15), insn(JMP | JEQ | K, 0, 1, q), insn(RET | K, k=65535), insn(RET | K, k=0),
    ])


CASES = {
    "ret1": [bpf.program([insn(RET | K, k=1)])],
    "tcp_port": [bpf.tcp_dst_port(PORT)],
    "ip_ip6_port": [ip_ip6_port(PORT)],
    "classify16": [classify(q) for q in range(16)],
}
assert len(CASES["ip_ip6_port"][0]) == 30
for progs in CASES.values():
    for p in progs:
        assert abi.bpf_validate(p)

dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)
data, offsets, caplens = to_device(b, dev)
total = int(b.caplens.sum(dtype=np.uint64))
matched = torch.empty(n, dtype=torch.uint8, device=dev)
bucket = torch.empty(n, dtype=torch.uint8, device=dev)
ret = torch.empty(n, dtype=torch.int32, device=dev)
totals = torch.zeros(abi.BPF_TOTALS, dtype=torch.int64, device=dev)
tuples = torch.empty(n * 48, dtype=torch.uint8, device=dev)
rng = np.random.default_rng(1)
sample = np.sort(rng.choice(n, size=min(args.sample, n), replace=False))


def timed(fn) -> dict:
    """`runs` runs of: warm-up, then `launches` launches, each between its own events, the median in ms."""
    medians = []
    for _ in range(runs):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
        for a, z in ev:
            a.record(st)
            fn()
            z.record(st)
        torch.cuda.synchronize()
        medians.append(statistics.median(a.elapsed_time(z) for a, z in ev))
    return {"ms": round(statistics.median(medians), 4), "min_ms": round(min(medians), 4),
            "max_ms": round(max(medians), 4), "run_medians_ms": [round(m, 4) for m in medians]}


def check(progs) -> dict:
    """The last launch's columns on the sample against pcppx_bpf_reference over the same descriptors."""
    m, bk, rv = matched.cpu().numpy(), bucket.cpu().numpy(), ret.cpu().numpy().view(np.uint32)
    tot = totals.cpu().numpy().view(np.uint64)
    assert int(tot[abi.BPF_MATCHED]) == int(m.sum(dtype=np.uint64)) and int(tot[abi.BPF_BAD_DESC]) == 0, tot.tolist()
    offs, caps = np.ascontiguousarray(b.offsets[sample]), np.ascontiguousarray(b.caplens[sample])
    k = len(sample)
    rm, rb, rr = np.empty(k, np.uint8), np.empty(k, np.uint8), np.empty(k, np.uint32)
    rt = np.empty(abi.BPF_TOTALS, np.uint64)
    rbatch = abi.Batch(b.data.ctypes.data, offs.ctypes.data, caps.ctypes.data, int(b.data.nbytes), k, b.linktype, 0)
    abi.bpf_reference(progs, rbatch, None, abi.BpfVerdicts(rm.ctypes.data, rb.ctypes.data, rr.ctypes.data,
                                                           rt.ctypes.data))
    assert np.array_equal(m[sample], rm) and np.array_equal(bk[sample], rb) and np.array_equal(rv[sample], rr)
    # and the reference's count over the whole batch (no columns)
    ft = np.empty(abi.BPF_TOTALS, np.uint64)
    abi.bpf_reference(progs, b.c_batch(), None, abi.BpfVerdicts(None, None, None, ft.ctypes.data))
    assert ft.tolist() == tot.tolist(), (ft.tolist(), tot.tolist())
    return {"matched": int(tot[abi.BPF_MATCHED]), "sample": k, "sample_matched": int(rt[abi.BPF_MATCHED])}


popts = abi.make_opts(0, 8, False, 0, window=abi.WINDOW_SHORT)
parse = timed(lambda: eng.parse_device(data, offsets, caplens, n, b.linktype, popts, None, None, st.cuda_stream,
                                       tuples=tuples))
parse["Mpps"] = round(n / parse["ms"] / 1e3, 1)

results = []
for name, progs in CASES.items():
    if args.only and args.only != name:
        continue
    with eng.bpf_load(progs) as flt:
        run = lambda: eng.bpf_device(flt, data, offsets, caplens, n, b.linktype, totals, matched, bucket, ret, None,  # noqa: E731
                                     st.cuda_stream)
        t = timed(run)
        torch.cuda.synchronize()
    t.update({"case": name, "programs": len(progs), "instructions": int(sum(len(p) for p in progs)),
              "Mpps": round(n / t["ms"] / 1e3, 1), "ratio_to_parse": round(t["ms"] / parse["ms"], 3)})
    if not args.no_check:
        t["checked_against_reference"] = check(progs)
    results.append(t)
doc = {"kernel": "bpf_kernel (one launch + the totals memset)", "packets": n, "batch_bytes": total, "port": PORT,
       "launches_per_run": launches, "runs": runs,
       "statistic": "median over runs of the per-run median of per-launch HIP event times; min / max over the runs",
       "parse_short_tuples": parse, "cases": results}
Path(args.out).parent.mkdir(parents=True, exist_ok=True)
Path(args.out).write_text(json.dumps(doc) + "\n")
print(json.dumps(doc))
eng.close()
