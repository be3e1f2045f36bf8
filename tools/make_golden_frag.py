"""Freeze the input fixture of pcppx_frag's reference vectors (tests/golden/frag/, run where the reference's data is).

The reference's own IPFragUtil tests (Tests/ExamplesTest/tests/test_ipfragutil.py) fragment pcap_examples/http-packets.pcap
at 256 bytes twice: the packets with IP id 22574 or 22582 (-d), and the packets a `tcp src port 8881` filter matches (-f).
Their expected outputs are small and already sit in tests/golden/ingest/files; the 2.7 MB input capture does not. This
tool reads that capture (a data file of the reference's tests; no program text is read or copied) and keeps the packets
the two runs split together with their two neighbours on each side -- unselected packets, and packets under the
fragment size -- as one small pcap, in capture order, timestamps and frame lengths kept:

  python tools/make_golden_frag.py
Writes tests/golden/frag/http_packets_subset.pcap.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from pcapplusplus_amd.pcap import from_packets, read_pcap, write_pcap  # noqa: E402

SOURCE = Path("/root/reference/Tests/ExamplesTest/pcap_examples/http-packets.pcap")
OUT = ROOT / "tests" / "golden" / "frag"
IP_IDS = (22574, 22582)
SRC_PORT = 8881
FRAG_SIZE = 256
NEIGHBOURS = 2


def chosen(p: bytes) -> bool:
    """Ethernet / IPv4 packets of either run's selection whose IP payload exceeds the fragment size."""
    if len(p) < 34 or p[12:14] != b"\x08\x00" or p[14] >> 4 != 4:
        return False
    hdr = (p[14] & 15) * 4
    total = int.from_bytes(p[16:18], "big")
    ipid = int.from_bytes(p[18:20], "big")
    tcp = p[23] == 6 and len(p) >= 14 + hdr + 2
    sport = int.from_bytes(p[14 + hdr:16 + hdr], "big") if tcp else -1
    return (ipid in IP_IDS or sport == SRC_PORT) and min(total, len(p) - 14) - hdr > FRAG_SIZE


def main() -> None:
    if not SOURCE.exists():
        raise SystemExit(f"{SOURCE} missing: the reference's test data is needed")
    b = read_pcap(SOURCE)
    take = sorted({j for i in range(b.n) if chosen(b.packet(i))
                   for j in range(max(i - NEIGHBOURS, 0), min(i + NEIGHBOURS + 1, b.n))})
    out = from_packets([b.packet(i) for i in take], b.linktype)
    out.timestamps_ns = b.timestamps_ns[take]
    out.frame_lens = b.frame_lens[take]
    OUT.mkdir(parents=True, exist_ok=True)
    write_pcap(OUT / "http_packets_subset.pcap", out)
    print(len(take), "of", b.n, "packets,", int(np.sum([chosen(b.packet(i)) for i in take])), "to split")


if __name__ == "__main__":
    main()
