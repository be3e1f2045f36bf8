"""Examples/TLSFingerprinting over a capture file, on the device: capture file in, the example's output file out.

  python tools/tlsfp_file.py -r capture.pcap [-o out.txt] [-t ch|sh|ch_sh] [-s SEPARATOR]

The capture is read by the project's reader, copied to HBM, parsed there (pcppx_parse_batch_device, with the 5-tuple
extracts) and fingerprinted there (pcppx_tlsfp_device); the records, the texts and the tuples come back and are written
as the example writes them (main.cpp:202-221): one row per ClientHello / ServerHello packet with the MD5, the
fingerprint, its kind, and the addresses and TCP ports. The summary the example prints follows on stdout
(main.cpp:277-322). Packets whose TLS layers the device parse leaves to the host (disposition HOST) are counted and
named; the example's -f BPF filter is pcppx_bpf_device's job and is not repeated here.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pcapplusplus_amd import abi, tlsfp  # noqa: E402
from pcapplusplus_amd.engine import Engine, tlsfp_on_device  # noqa: E402
from pcapplusplus_amd.pcap import read_pcap  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-r", "--input", required=True, help="pcap file to read")
    ap.add_argument("-o", "--output", help="output file (default: <input>.txt)")
    ap.add_argument("-t", "--type", choices=("ch", "sh", "ch_sh"), default="ch",
                    help="ClientHello, ServerHello or both fingerprints (default: ch)")
    ap.add_argument("-s", "--separator", default="\t", help="column separator of the output file (default: a tab)")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if len(a.separator) != 1 or a.separator in "-,":
        raise SystemExit("the separator is one character, not one the fingerprint itself uses")
    client, server = a.type in ("ch", "ch_sh"), a.type in ("sh", "ch_sh")
    batch = read_pcap(a.input)
    with Engine(a.device) as eng:
        recs, text, tuples, disp, tot = tlsfp_on_device(eng, batch, client, server, device=f"cuda:{a.device}")
    out = a.output or a.input + ".txt"
    tlsfp.write_rows(out, tlsfp.rows(recs, tuples, text), a.separator)
    print("\nSummary:\n========")
    print(f"Total packets read:                   {batch.n}")
    for want, kind, name, count in ((client, abi.TLSFP_CLIENT, "ClientHello", tot["client_n"]),
                                    (server, abi.TLSFP_SERVER, "ServerHello", tot["server_n"])):
        if not want:
            continue
        table = tlsfp.top(recs, kind, None)
        print(f"TLS {name} packets:              {count}")
        print(f"Unique {name} TLS fingerprints:  {len(table)}")
    if tot["host_n"] or tot["bad_desc"]:
        print(f"Packets left to a host parse:         {tot['host_n']} (bad descriptors: {tot['bad_desc']})")
    for want, kind, name in ((client, abi.TLSFP_CLIENT, "ClientHello"), (server, abi.TLSFP_SERVER, "ServerHello")):
        table = tlsfp.top(recs, kind, None) if want else []
        if not table:
            continue
        print(("\nTop 10 " if len(table) > 10 else "\n") + f"{name} TLS fingerprints:")
        for md5, count in table[:10]:
            print(f"{md5} | {count}")
    print(f"\nOutput file was written to: {out}")


if __name__ == "__main__":
    main()
