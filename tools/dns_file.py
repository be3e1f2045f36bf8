"""DnsLayer's resources of a capture file: capture file in, one row per linked resource out.

  python tools/dns_file.py -r capture.pcap [-o out.txt] [--sections 15] [--count] [--reference]

The capture is read by the project's reader, copied to HBM, parsed there (pcppx_parse_batch_device) and its DNS
messages are walked there (pcppx_dns_device); the messages, the resource records and the names come back and are written
one row per resource: the packet's number, the section, the decoded name, type, class, TTL and data length. --count
prints what the dns mode of Examples/PcapPlusPlus-benchmark prints first (`benchmark <file> dns 1`): the linked queries
plus answers of all messages. --reference runs without a GPU: the parse's restatement (oracle/) writes the records and
pcppx_dns_reference walks the messages. Packets whose DNS layer the device parse leaves to the host (disposition HOST)
are counted and named.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pcapplusplus_amd import abi, dns  # noqa: E402
from pcapplusplus_amd.pcap import read_pcap  # noqa: E402


def on_host(batch, sections: int):
    """(msgs, rrs, names, totals) through oracle.oracle_parse and pcppx_dns_reference."""
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
    spec = abi.make_dns_spec(sections)
    totals = np.zeros(abi.DNS_TOTALS, np.uint64)

    def call(msgs, rrs, names):
        o = abi.DnsOut(msgs.ctypes.data, rrs.ctypes.data, names.ctypes.data, len(names), None, len(msgs) - 1,
                       len(rrs) - 1, totals.ctypes.data)
        abi.dns_reference(b, r, ml, spec, o)
        return abi.dns_totals_dict(totals)

    empty = lambda k, dt: np.zeros(k + 1, dt)  # noqa: E731  (one entry more than the room: never a null pointer)
    need = call(empty(0, abi.DNS_MSG_DTYPE), empty(0, abi.DNS_RR_DTYPE), np.zeros(0, np.uint8))
    msgs, rrs = empty(need["msgs"], abi.DNS_MSG_DTYPE), empty(need["rrs"], abi.DNS_RR_DTYPE)
    names = np.zeros(need["name_bytes"], np.uint8)
    tot = call(msgs, rrs, names) if need["overflow"] else need
    assert tot["overflow"] == 0
    return msgs[:tot["msgs"]], rrs[:tot["rrs"]], names, tot


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-r", "--input", required=True, help="pcap file to read")
    ap.add_argument("-o", "--output", help="output file (default: <input>.dns.txt)")
    ap.add_argument("--sections", type=int, default=15, help="bit 0 queries, 1 answers, 2 authorities, 3 additionals")
    ap.add_argument("--count", action="store_true", help="print only the linked queries plus answers")
    ap.add_argument("--reference", action="store_true", help="no GPU: the restatement's records, pcppx_dns_reference")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if not 1 <= a.sections <= 15:
        raise SystemExit("--sections is 1..15")
    batch = read_pcap(a.input)
    if a.reference:
        msgs, rrs, names, tot = on_host(batch, a.sections)
    else:
        from pcapplusplus_amd.engine import Engine, dns_on_device

        with Engine(a.device) as eng:
            msgs, rrs, names, _, tot = dns_on_device(eng, batch, a.sections, device=f"cuda:{a.device}")
    if a.count:
        print(tot["qa_linked"])
        return
    out = a.output or a.input + ".dns.txt"
    with open(out, "w") as f:
        for row in dns.rows(msgs, rrs, names):
            f.write(dns.format_row(row) + "\n")
    print(f"Total packets read:      {batch.n}")
    print(f"DNS messages:            {tot['msgs']}")
    print(f"Resource records:        {tot['rrs']}")
    print(f"Queries plus answers:    {tot['qa_linked']}")
    if tot["host_n"] or tot["bad_desc"]:
        print(f"Packets left to a host parse: {tot['host_n']} (bad descriptors: {tot['bad_desc']})")
    print(f"Output file was written to: {out}")


if __name__ == "__main__":
    main()
