"""Time of pcppx_dhcp_device on a device-resident batch, beside the device parse of the same batch and the single-core
time of pcppx_dhcp_reference.

  python tools/bench_dhcp.py [packets] [launches] [out.json]

Workload: config-3 IMIX (64 / 512 / 1500 B at 7:4:1, 25 % VLAN, 30 % IPv6), `packets` of it (1M by default), of which
a share of 1 % and 100 % (evenly spread) is replaced by DHCP packets from pcapplusplus_amd.dhcp's builders: 4096
distinct messages -- discover, offer, request and ack of 1024 clients in turn, every third message a DHCPv6 message
of the types 1..13 on the ports 546 / 547, one DHCPv4 message in nine with PAD bytes behind END. The batch is resident
in HBM and parsed once (summary, FIXED layers); the spec asks for the option records of the DHCPv4 codes 12, 50, 51, 53,
54, 55, 60, 61 and the DHCPv6 codes 1, 2, 3, 39 (WANTED) with their values, the dispositions written; the buffers are
sized by a call without room, as a caller would.
Method: after 3 warm-up launches, `launches` (>= 50) launches, each between its own pair of HIP events on the launch
stream, nothing else running on the device; the median, the minimum and the maximum of the per-launch times are given.
A launch is the whole call: the plan, base and emit kernels in stream order. The parse of the same batch is timed the
same way in the same process. pcppx_dhcp_reference runs once on one core over the same batch and records, and the
device's output is compared with its output in every row. There is no earlier implementation to compare with: the file
holds what was measured.
Prints one JSON line (and writes it into out.json when given).
"""
import json
import statistics
import struct
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from pcapplusplus_amd import abi, dhcp, synth  # noqa: E402
from pcapplusplus_amd.engine import Engine, to_device  # noqa: E402
from pcapplusplus_amd.pcap import PacketBatch, from_packets  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
launches = max(int(sys.argv[2]) if len(sys.argv) > 2 else 50, 50)
out_path = (sys.argv[3] if len(sys.argv) > 3 else None) or None

ML = 8
SHARES = (0.01, 1.0)
POOL = 4096
PARAMS = bytes((1, 3, 6, 15, 31, 33, 43, 44, 46, 47, 119, 121, 249, 252))
dev = "cuda:0"
eng = Engine(0)
st = torch.cuda.current_stream(dev)


def dhcp_packet(k: int) -> bytes:
    c = k // 4
    mac = bytes((2, 0, 0, 0, (c >> 8) & 255, c & 255))
    addr = bytes((10, 0, (c >> 8) & 255, c & 255))
    if k % 3 == 2:
        duid = b"\x00\x01\x00\x01" + struct.pack(">I", c) + mac
        msg = dhcp.message6(1 + k % 13, 0x100000 + k, [(1, duid), (3, struct.pack(">III", c, 0, 0)),
                                                        (6, bytes((0, 23, 0, 24))), (39, b"\0\x05host" + b"%d" % c)])
        return dhcp.packet(msg, k, *((546, 547) if k % 2 else (547, 546)))
    kind = k % 4
    if kind == 0:
        o = [(61, b"\x01" + mac), (12, b"host-%d" % c), (60, b"MSFT 5.0"), (55, PARAMS)]
    elif kind == 2:
        o = [(61, b"\x01" + mac), (50, addr), (54, bytes((10, 0, 0, 1))), (12, b"host-%d" % c), (55, PARAMS[:9])]
    else:
        o = [(54, bytes((10, 0, 0, 1))), (51, struct.pack(">I", 3600 + c)), (1, bytes((255, 255, 255, 0))),
             (3, bytes((10, 0, 0, 1))), (6, bytes((8, 8, 8, 8, 8, 8, 4, 4)))]
    msg = dhcp.message4((dhcp.DISCOVER, dhcp.OFFER, dhcp.REQUEST, dhcp.ACK)[kind], o, xid=0x1000 + c, mac=mac,
                        yiaddr=".".join(str(x) for x in addr) if kind & 1 else "0.0.0.0")
    msg += bytes(k % 40) if k % 9 == 0 else b""
    return dhcp.packet(msg, k, *((67, 68) if kind & 1 else (68, 67)))


def with_dhcp(b: PacketBatch, pool: PacketBatch, share: float) -> PacketBatch:
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
pool = from_packets([dhcp_packet(k) for k in range(POOL)])
spec = abi.make_dhcp_spec(abi.DHCP_ASSET_CODES4, abi.DHCP_ASSET_CODES6, abi.DHCP_OPTIONS_WANTED, 1)
results = []
for share in SHARES:
    b = with_dhcp(imix, pool, share)
    data, offsets, caplens = to_device(b, dev)
    summary = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    layers = torch.empty(n * ML * 8, dtype=torch.uint8, device=dev)
    opts = abi.make_opts(0, 8, False, ML)
    parse = lambda: eng.parse_device(data, offsets, caplens, n, b.linktype, opts, summary, layers,  # noqa: E731
                                     st.cuda_stream)
    parse()
    totals = torch.zeros(abi.DHCP_TOTALS, dtype=torch.int64, device=dev)
    one = torch.empty(80, dtype=torch.uint8, device=dev)
    eng.dhcp_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, one, one, totals, 0, 0,
                    stream=st.cuda_stream, summary=summary)
    torch.cuda.synchronize()
    need = abi.dhcp_totals_dict(totals.cpu().numpy().view(np.uint64))
    m, k, nb = need["msgs"], need["options"], need["value_bytes"]
    msgs = torch.empty(max(m, 1) * 80, dtype=torch.uint8, device=dev)
    options = torch.empty(max(k, 1) * 16, dtype=torch.uint8, device=dev)
    values = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
    disp = torch.empty(n, dtype=torch.uint8, device=dev)
    run = lambda: eng.dhcp_device(data, offsets, caplens, n, b.linktype, layers, ML, spec, msgs, options, totals,  # noqa: E731
                                  m, k, values, nb, disp, st.cuda_stream, summary=summary)
    for _ in range(3):
        run()
        parse()
    torch.cuda.synchronize()
    tot = abi.dhcp_totals_dict(totals.cpu().numpy().view(np.uint64))
    assert tot["overflow"] == 0 and tot["msgs"] == m
    t_ms = per_launch(run, launches)
    p_ms = per_launch(parse, launches)
    # the same batch and records through the host reference, one core
    h_sum, h_lay = summary.cpu().numpy(), layers.cpu().numpy()
    h_msgs, h_options = np.empty(max(m, 1) * 80, np.uint8), np.empty(max(k, 1) * 16, np.uint8)
    h_values, h_disp, h_tot = np.empty(nb + 64, np.uint8), np.empty(n, np.uint8), np.zeros(abi.DHCP_TOTALS, np.uint64)
    hb = abi.Batch(b.data.ctypes.data, b.offsets.ctypes.data, b.caplens.ctypes.data, len(b.data), n, b.linktype, 0)
    ho = abi.DhcpOut(h_msgs.ctypes.data, h_options.ctypes.data, h_values.ctypes.data, nb, h_disp.ctypes.data, m, k, 0,
                     h_tot.ctypes.data)
    t0 = time.perf_counter()
    abi.dhcp_reference(hb, abi.Records(h_sum.ctypes.data, h_lay.ctypes.data), ML, spec, ho)
    ref_ms = (time.perf_counter() - t0) * 1e3
    same = bool((msgs.cpu().numpy()[:m * 80] == h_msgs[:m * 80]).all() and
                (options.cpu().numpy()[:k * 16] == h_options[:k * 16]).all() and
                (values.cpu().numpy()[:nb] == h_values[:nb]).all() and (disp.cpu().numpy() == h_disp).all() and
                list(totals.cpu().numpy().view(np.uint64)) == list(h_tot))
    med = statistics.median(t_ms)
    results.append({"dhcp_share": share, "options": "WANTED", "packets": n, "messages": m, "v4": tot["v4"],
                    "v6": tot["v6"], "records": k, "value_bytes": nb, "options_linked": tot["options_linked"],
                    "host_n": tot["host_n"], "dhcp": stats(t_ms), "Mpps": round(n / med / 1e3, 1),
                    "messages_per_us": round(m / med / 1e3, 2), "parse": stats(p_ms),
                    "dhcp_over_parse": round(med / statistics.median(p_ms), 3),
                    "reference_one_core_ms": round(ref_ms, 2), "device_equals_reference": same})
    del msgs, options, values, disp, data, offsets, caplens, summary, layers
    torch.cuda.empty_cache()
entry = {"kernel": "dhcp (plan + bases + emit)", "launches_per_case": launches, "warmup_launches": 3,
         "timing": "one HIP event pair per launch, median of the launches", "cases": results}
print(json.dumps(entry))
if out_path:
    p = Path(out_path)
    p.parent.mkdir(parents=True, exist_ok=True)
    p.write_text(json.dumps(entry) + "\n")
eng.close()
assert all(r["device_equals_reference"] for r in results)
