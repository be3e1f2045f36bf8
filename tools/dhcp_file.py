"""The DHCP and DHCPv6 messages of a capture file: capture file in, one row per message and wanted option, the lease
table or the client fingerprints out.

  python tools/dhcp_file.py -r capture.pcap [-o out.txt] [--codes4 12,50,...] [--codes6 1,2,...] [--all]
                            [--leases | --fingerprints] [--reference]

The capture is read by the project's reader, copied to HBM, parsed there (pcppx_parse_batch_device) and its DHCP /
DHCPv6 messages are walked there (pcppx_dhcp_device); the messages, the option records and the values come back.
Without --leases / --fingerprints one row per message and one per option record is written: the packet's number, the
family, the message type, then the option count, or the option's code, length and value. --leases prints the MAC <->
address <-> lease table of the DHCPv4 ACKs as JSON (pcapplusplus_amd.dhcp.leases), --fingerprints the option 55 list and
the option 60 text of every DHCPv4 DISCOVER / REQUEST (pcapplusplus_amd.dhcp.fingerprints). --reference runs without a
GPU: the parse's restatement (oracle/) writes the records and pcppx_dhcp_reference walks the messages. Packets whose
answer is left to the host (disposition HOST) are counted and named.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pcapplusplus_amd import abi, dhcp  # noqa: E402
from pcapplusplus_amd.pcap import read_pcap  # noqa: E402


def on_host(batch, spec: abi.DhcpSpec):
    """(msgs, options, values, totals) through oracle.oracle_parse and pcppx_dhcp_reference."""
    import oracle

    opts = abi.make_opts()
    n, ml = batch.n, opts.max_layers
    summary, layers = oracle.oracle_parse(batch, opts)
    summary = np.ascontiguousarray(summary) if n else np.zeros(1, abi.SUMMARY_DTYPE)
    layers = np.ascontiguousarray(layers) if n else np.zeros(ml, abi.LAYER_DTYPE)
    data = batch.data if len(batch.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, batch.offsets.ctypes.data, batch.caplens.ctypes.data, len(batch.data), n,
                  batch.linktype, 0)
    r = abi.Records(summary.ctypes.data, layers.ctypes.data)
    totals = np.zeros(abi.DHCP_TOTALS, np.uint64)

    def call(msgs, options, values):
        o = abi.DhcpOut(msgs.ctypes.data, options.ctypes.data, values.ctypes.data, len(values), None, len(msgs) - 1,
                        len(options) - 1, 0, totals.ctypes.data)
        abi.dhcp_reference(b, r, ml, spec, o)
        return abi.dhcp_totals_dict(totals)

    empty = lambda k, dt: np.zeros(k + 1, dt)  # noqa: E731  (one entry more than the room: never a null pointer)
    need = call(empty(0, abi.DHCP_MSG_DTYPE), empty(0, abi.DHCP_OPTION_DTYPE), np.zeros(0, np.uint8))
    msgs, options = empty(need["msgs"], abi.DHCP_MSG_DTYPE), empty(need["options"], abi.DHCP_OPTION_DTYPE)
    values = np.zeros(need["value_bytes"], np.uint8)
    tot = call(msgs, options, values) if need["overflow"] else need
    assert tot["overflow"] == 0
    return msgs[:tot["msgs"]], options[:tot["options"]], values, tot


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-r", "--input", required=True, help="pcap file to read")
    ap.add_argument("-o", "--output", help="output file (default: <input>.dhcp.txt)")
    ap.add_argument("--codes4", default=",".join(str(c) for c in abi.DHCP_ASSET_CODES4), help="wanted DHCPv4 codes")
    ap.add_argument("--codes6", default=",".join(str(c) for c in abi.DHCP_ASSET_CODES6),
                    help="up to 16 wanted DHCPv6 codes")
    ap.add_argument("--all", action="store_true", help="a row for every option (PAD and END too)")
    ap.add_argument("--leases", action="store_true", help="print the lease table as JSON (needs 12 among --codes4)")
    ap.add_argument("--fingerprints", action="store_true", help="print the client fingerprints as JSON (needs 55, 60)")
    ap.add_argument("--reference", action="store_true", help="no GPU: the restatement's records, pcppx_dhcp_reference")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    codes = lambda text: tuple(sorted({int(x) for x in text.split(",") if x}))  # noqa: E731
    spec = abi.make_dhcp_spec(codes(a.codes4), codes(a.codes6),
                              abi.DHCP_OPTIONS_ALL if a.all else abi.DHCP_OPTIONS_WANTED, 1)
    batch = read_pcap(a.input)
    if a.reference:
        msgs, options, values, tot = on_host(batch, spec)
    else:
        from pcapplusplus_amd.engine import Engine, dhcp_on_device

        with Engine(a.device) as eng:
            msgs, options, values, _, tot = dhcp_on_device(eng, batch, spec, device=f"cuda:{a.device}")
    if a.leases or a.fingerprints:
        table = dhcp.leases if a.leases else dhcp.fingerprints
        print(json.dumps(table(msgs, options, values), indent=1, sort_keys=True))
        return
    out = a.output or a.input + ".dhcp.txt"
    with open(out, "w") as f:
        for row in dhcp.rows(msgs, options, values):
            f.write(dhcp.format_row(row) + "\n")
    print(f"Total packets read:      {batch.n}")
    print(f"DHCP messages:           {tot['v4']} ({tot['replies']} replies)")
    print(f"DHCPv6 messages:         {tot['v6']}")
    print(f"Options:                 {tot['options_linked']} ({tot['options']} rows, {tot['value_bytes']} value bytes)")
    if tot["host_n"] or tot["bad_desc"]:
        print(f"Packets left to a host parse: {tot['host_n']} (bad descriptors: {tot['bad_desc']})")
    print(f"Output file was written to: {out}")


if __name__ == "__main__":
    main()
