"""Freeze the fixtures of pcppx_defrag6's tests (tests/golden/defrag6/, run where the reference's data is).

Two kinds of data, no program text:

  * ip6_fragments_packet1.txt / ip6_fragments_packet2.txt: the reassembled packets the reference's own tests expect of
    Tests/Pcap++Test/PcapExamples/ip6_fragments.pcap (the capture is already in tests/golden/ingest/files), copied.
  * expected.npz: for the crafted quirk shapes of tests/defrag6_cases.py (quirk_cases()), the fragments as they were fed
    to the reference's IPReassembly::processPacket, in order, and the packet it returned with REASSEMBLED (or nothing).
    The recording itself is made by a stand-alone program linked against a build of the reference, which is not part of
    this repository: it reads the file --inputs writes (u32 cases; per case u32 packets; per packet u32 length and the
    bytes) and writes the file --recorded reads (u32 cases; per case u32 results; per result u32 arrival number, u32
    length and the bytes).

  python tools/make_golden_defrag6.py --inputs quirks.in
  <the recorder> quirks.in quirks.out
  python tools/make_golden_defrag6.py --recorded quirks.out
"""
from __future__ import annotations

import argparse
import shutil
import struct
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

SOURCE = Path("/root/reference/Tests/Pcap++Test/PcapExamples")
OUT = ROOT / "tests" / "golden" / "defrag6"
VECTORS = ("ip6_fragments_packet1.txt", "ip6_fragments_packet2.txt")


def quirk_packets():
    import defrag6_cases as d6

    return [(c.name, [c.batch().packet(i) for i in range(c.n)]) for c in d6.quirk_cases()]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--inputs", type=Path)
    ap.add_argument("--recorded", type=Path)
    args = ap.parse_args()
    OUT.mkdir(parents=True, exist_ok=True)
    cases = quirk_packets()
    if args.inputs:
        with open(args.inputs, "wb") as f:
            f.write(struct.pack("<I", len(cases)))
            for _, pk in cases:
                f.write(struct.pack("<I", len(pk)))
                for p in pk:
                    f.write(struct.pack("<I", len(p)) + p)
        print(len(cases), "cases written to", args.inputs)
    if args.recorded:
        raw = args.recorded.read_bytes()
        at = 4
        assert struct.unpack_from("<I", raw)[0] == len(cases)
        arrays = {}
        for name, pk in cases:
            nres, = struct.unpack_from("<I", raw, at)
            at += 4
            assert nres <= 1, name
            arrays[f"{name}.lens"] = np.array([len(p) for p in pk], np.uint32)
            arrays[f"{name}.packets"] = np.frombuffer(b"".join(pk), np.uint8)
            arrays[f"{name}.at"] = np.array([-1], np.int32)
            arrays[f"{name}.out"] = np.zeros(0, np.uint8)
            for _ in range(nres):
                idx, ln = struct.unpack_from("<II", raw, at)
                at += 8
                arrays[f"{name}.at"] = np.array([idx], np.int32)
                arrays[f"{name}.out"] = np.frombuffer(raw[at:at + ln], np.uint8)
                at += ln
            print(name, "reassembled on arrival", int(arrays[f"{name}.at"][0]), len(arrays[f"{name}.out"]), "bytes")
        assert at == len(raw)
        np.savez_compressed(OUT / "expected.npz", **arrays)
    if SOURCE.exists():
        for v in VECTORS:
            shutil.copyfile(SOURCE / v, OUT / v)
    elif not all((OUT / v).exists() for v in VECTORS):
        raise SystemExit(f"{SOURCE} missing: the reference's test data is needed")


if __name__ == "__main__":
    main()
