"""The SIP messages of a capture file: capture file in, one row per wanted header field or the per-call table out.

  python tools/sip_file.py -r capture.pcap [-o out.txt] [--names call-id,from,to,cseq] [--all] [--calls] [--reference]

The capture is read by the project's reader, copied to HBM, parsed there (pcppx_parse_batch_device) and its SIP
messages are walked there (pcppx_sip_device); the messages, the field records, the SDP records and the text come back.
Without --calls one row per field record is written: the packet's number, request or response, the name's number in
--names (255 for another name, with --all), the flags, the name's and the value's length and the value. --calls prints
the per-Call-ID table as one JSON object instead (pcapplusplus_amd.sip.calls): per call its packets, the method and
status-code counts, and the SDP owner addresses and RTP ports seen. --reference runs without a GPU: the parse's
restatement (oracle/) writes the records and pcppx_sip_reference walks the messages. Packets whose SIP answer is left
to the host (disposition HOST) are counted and named.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pcapplusplus_amd import abi, sip  # noqa: E402
from pcapplusplus_amd.pcap import read_pcap  # noqa: E402


def on_host(batch, spec: abi.SipSpec):
    """(msgs, fields, sdps, text, totals) through oracle.oracle_parse and pcppx_sip_reference."""
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
    totals = np.zeros(abi.SIP_TOTALS, np.uint64)

    def call(msgs, fields, sdps, text):
        o = abi.SipOut(msgs.ctypes.data, fields.ctypes.data, sdps.ctypes.data, text.ctypes.data, len(text), None,
                       len(msgs) - 1, len(fields) - 1, len(sdps) - 1, 0, totals.ctypes.data)
        abi.sip_reference(b, r, ml, spec, o)
        return abi.sip_totals_dict(totals)

    empty = lambda k, dt: np.zeros(k + 1, dt)  # noqa: E731  (one entry more than the room: never a null pointer)
    need = call(empty(0, abi.SIP_MSG_DTYPE), empty(0, abi.SIP_FIELD_DTYPE), empty(0, abi.SIP_SDP_DTYPE),
                np.zeros(0, np.uint8))
    msgs, fields = empty(need["msgs"], abi.SIP_MSG_DTYPE), empty(need["fields"], abi.SIP_FIELD_DTYPE)
    sdps, text = empty(need["sdps"], abi.SIP_SDP_DTYPE), np.zeros(need["text_bytes"], np.uint8)
    tot = call(msgs, fields, sdps, text) if need["overflow"] else need
    assert tot["overflow"] == 0
    return msgs[:tot["msgs"]], fields[:tot["fields"]], sdps[:tot["sdps"]], text, tot


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-r", "--input", required=True, help="pcap file to read")
    ap.add_argument("-o", "--output", help="output file (default: <input>.sip.txt)")
    ap.add_argument("--names", default=",".join(abi.SIP_CALL_NAMES), help="up to 8 field names, lower case")
    ap.add_argument("--all", action="store_true", help="a row for every field, not only for those in --names")
    ap.add_argument("--calls", action="store_true", help="print the per-call table as JSON (needs call-id among "
                    "--names)")
    ap.add_argument("--reference", action="store_true", help="no GPU: the restatement's records, pcppx_sip_reference")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    names = tuple(x for x in a.names.split(",") if x)
    spec = abi.make_sip_spec(names, abi.HTTP_FIELDS_ALL if a.all else abi.HTTP_FIELDS_WANTED, 3)
    batch = read_pcap(a.input)
    if a.reference:
        msgs, fields, sdps, text, tot = on_host(batch, spec)
    else:
        from pcapplusplus_amd.engine import Engine, sip_on_device

        with Engine(a.device) as eng:
            msgs, fields, sdps, text, _, tot = sip_on_device(eng, batch, spec, device=f"cuda:{a.device}")
    if a.calls:
        print(json.dumps(sip.calls(msgs, fields, sdps, text, names), indent=1, sort_keys=True))
        return
    out = a.output or a.input + ".sip.txt"
    with open(out, "w") as f:
        for row in sip.rows(msgs, fields, text):
            f.write(sip.format_row(row) + "\n")
    print(f"Total packets read:      {batch.n}")
    print(f"SIP requests:            {tot['requests']}")
    print(f"SIP responses:           {tot['responses']}")
    print(f"By the heuristic path:   {tot['by_heuristic']}")
    print(f"SDP bodies:              {tot['sdps']}")
    print(f"Header fields:           {tot['fields_linked']} ({tot['fields']} rows)")
    if tot["host_n"] or tot["bad_desc"]:
        print(f"Packets left to a host parse: {tot['host_n']} (bad descriptors: {tot['bad_desc']})")
    print(f"Output file was written to: {out}")


if __name__ == "__main__":
    main()
