"""The SSL/TLS packets of a capture file: capture file in, one row per hello or SSLAnalyzer's tables out.

  python tools/ssl_file.py -r capture.pcap [-o out.txt] [--kinds 3] [--analyze] [--reference]

The capture is read by the project's reader, copied to HBM, parsed there (pcppx_parse_batch_device) and its SSL/TLS
records are walked there (pcppx_ssl_device); the messages, the hello records and the host names come back. Without
--analyze one row per hello record is written: the packet's number, client or server, the version, the cipher suite id,
the cipher count, the extension count, the session id's length, the flags and the SNI host name. --analyze prints the
tables of Examples/SSLAnalyzer as one JSON object instead (pcapplusplus_amd.ssl.analyze): packets, flows, data, hellos,
completed handshakes, alerts, ports, versions, cipher suite ids, host names. --reference runs without a GPU: the
parse's restatement (oracle/) writes the records and pcppx_ssl_reference walks them. Packets whose chain the device parse
leaves to the host (disposition HOST) are counted and named.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pcapplusplus_amd import abi  # noqa: E402
from pcapplusplus_amd import ssl as sl  # noqa: E402
from pcapplusplus_amd.pcap import read_pcap  # noqa: E402


def on_host(batch, spec: abi.SslSpec):
    """(msgs, hellos, names, hash5, totals) through oracle.oracle_parse and pcppx_ssl_reference."""
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
    totals = np.zeros(abi.SSL_TOTALS, np.uint64)

    def call(msgs, hellos, names):
        o = abi.SslOut(msgs.ctypes.data, hellos.ctypes.data, names.ctypes.data, len(names), None, len(msgs) - 1,
                       len(hellos) - 1, totals.ctypes.data)
        abi.ssl_reference(b, r, ml, spec, o)
        return abi.ssl_totals_dict(totals)

    empty = lambda k, dt: np.zeros(k + 1, dt)  # noqa: E731  (one entry more than the room: never a null pointer)
    need = call(empty(0, abi.SSL_MSG_DTYPE), empty(0, abi.SSL_HELLO_DTYPE), np.zeros(1, np.uint8)[:0])
    msgs, hellos = empty(need["msgs"], abi.SSL_MSG_DTYPE), empty(need["hellos"], abi.SSL_HELLO_DTYPE)
    names = np.zeros(need["name_bytes"] + 1, np.uint8)[:need["name_bytes"]]
    tot = call(msgs, hellos, names) if need["overflow"] else need
    assert tot["overflow"] == 0
    return msgs[:tot["msgs"]], hellos[:tot["hellos"]], names, summary["hash5"][:n], tot


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-r", "--input", required=True, help="pcap file to read")
    ap.add_argument("-o", "--output", help="output file (default: <input>.ssl.txt)")
    ap.add_argument("--kinds", type=int, default=3, help="bit 0 client hellos, bit 1 server hellos")
    ap.add_argument("--analyze", action="store_true", help="print SSLAnalyzer's tables as JSON (needs --kinds 3)")
    ap.add_argument("--reference", action="store_true", help="no GPU: the restatement's records, pcppx_ssl_reference")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    batch = read_pcap(a.input)
    if a.reference:
        msgs, hellos, names, hash5, tot = on_host(batch, abi.make_ssl_spec(a.kinds))
    else:
        from pcapplusplus_amd.engine import Engine, ssl_on_device

        with Engine(a.device) as eng:
            msgs, hellos, names, hash5, _, tot = ssl_on_device(eng, batch, a.kinds, device=f"cuda:{a.device}")
    if a.analyze:
        print(json.dumps(sl.analyze(msgs, hellos, names, hash5), indent=1, sort_keys=True))
        return
    out = a.output or a.input + ".ssl.txt"
    with open(out, "w") as f:
        for row in sl.rows(msgs, hellos, names):
            f.write(sl.format_row(row) + "\n")
    print(f"Total packets read:      {batch.n}")
    print(f"SSL packets:             {tot['msgs']} ({tot['payload_bytes']} bytes)")
    print(f"Client hellos:           {tot['client_hellos']}")
    print(f"Server hellos:           {tot['server_hellos']}")
    print(f"Packets with an alert:   {tot['alert_pkts']}")
    if tot["host_n"] or tot["bad_desc"]:
        print(f"Packets left to a host parse: {tot['host_n']} (bad descriptors: {tot['bad_desc']})")
    print(f"Output file was written to: {out}")


if __name__ == "__main__":
    main()
