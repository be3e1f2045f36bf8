"""Freeze the reference vectors of pcppx_tlsfp's tests (tests/golden/tlsfp/).

The reference's own TLSFingerprinting tests (Tests/ExamplesTest/tests/test_tlsfingerprinting.py) run the example over
pcap_examples/tls2.pcap (7,451 packets, 2.85 MB) and compare its output file with text files under expected_output.
This tool copies those data files -- no program text is read or copied:

  python tools/make_golden_tlsfp.py <the reference's Tests/ExamplesTest directory>

The three expected outputs (-t ch, sh and ch_sh) are copied as they are. The capture is larger than a committed file may
be, so tls2_handshakes.pcap holds a part of it, the records byte for byte and in the file's order: every packet whose
TCP payload starts with a TLS handshake or change-cipher-spec record (which is where every hello of the capture sits:
the three outputs keep all their 323 / 302 / 625 rows), and every 16th of the other packets, so that application data,
bare ACKs and non-TLS traffic stay in the batch.
"""
from __future__ import annotations

import shutil
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden" / "tlsfp"
CAPTURE = "pcap_examples/tls2.pcap"
TEXTS = ("expected_output/tls_fp_ch.txt", "expected_output/tls_fp_sh.txt", "expected_output/tls_fp_ch_sh.txt")
KEEP_EVERY = 16


def tcp_payload(pkt: bytes) -> bytes:
    """The TCP payload of an Ethernet / IPv4 or IPv6 / TCP packet (b"" for anything else)."""
    if len(pkt) < 14:
        return b""
    et, at = struct.unpack(">H", pkt[12:14])[0], 14
    if et == 0x0800 and len(pkt) >= at + 20 and pkt[at + 9] == 6:
        at += (pkt[at] & 15) * 4
    elif et == 0x86DD and len(pkt) >= at + 40 and pkt[at + 6] == 6:
        at += 40
    else:
        return b""
    if len(pkt) < at + 20:
        return b""
    return pkt[at + (pkt[at + 12] >> 4) * 4:]


def handshakes(src: Path, dst: Path) -> tuple[int, int]:
    raw = src.read_bytes()
    magic = struct.unpack("<I", raw[:4])[0]
    if magic not in (0xA1B2C3D4, 0xA1B23C4D):
        raise SystemExit(f"{src}: not a little-endian pcap file")
    out, at, k, kept, others = [raw[:24]], 24, 0, 0, 0
    while at + 16 <= len(raw):
        caplen = struct.unpack("<I", raw[at + 8:at + 12])[0]
        pkt = raw[at + 16:at + 16 + caplen]
        pay = tcp_payload(pkt)
        if len(pay) >= 3 and pay[0] in (20, 22) and pay[1] == 3:
            keep = True
        else:
            keep = others % KEEP_EVERY == 0
            others += 1
        if keep:
            out.append(raw[at:at + 16 + caplen])
            kept += 1
        at += 16 + caplen
        k += 1
    dst.write_bytes(b"".join(out))
    return k, kept


def main() -> None:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / CAPTURE).exists():
        raise SystemExit(__doc__)
    OUT.mkdir(parents=True, exist_ok=True)
    for name in TEXTS:
        dst = OUT / Path(name).name
        shutil.copyfile(Path(sys.argv[1]) / name, dst)
        dst.chmod(0o644)
        print(dst.name, dst.stat().st_size)
    dst = OUT / "tls2_handshakes.pcap"
    total, kept = handshakes(Path(sys.argv[1]) / CAPTURE, dst)
    print(dst.name, dst.stat().st_size, f"{kept} of {total} packets")


if __name__ == "__main__":
    main()
