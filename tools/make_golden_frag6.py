"""Freeze the fixture of pcppx_frag6's tests (tests/golden/frag6/expected.npz): data only, no program text.

For the crafted IPv6 packets of tests/frag6_cases.py (quirk_cases()), the fragments the reference's own routine makes
of them: the steps splitIPPacketToFragmentsBySize runs per fragment (Examples/IPFragUtil/main.cpp:
185-237) -- copy the RawPacket, removeAllLayersAfter, addLayer(PayloadLayer),
addExtension(IPv6FragmentationHeader(id, offset, last)), computeCalculateFields -- with the case's id in place of
rand(). The recording itself is made by a stand-alone program linked against a build of the reference, which is not
part of this repository: it reads the file --inputs writes (u32 cases; per case u32 fragment size, u32 id, u32 link
type, u32 length and the packet's bytes) and writes the file --recorded reads (u32 cases; per case u32 fragments; per
fragment u32 length and the bytes).

  python tools/make_golden_frag6.py --inputs quirks.in
  <the recorder> quirks.in quirks.out
  python tools/make_golden_frag6.py --recorded quirks.out
"""
from __future__ import annotations

import argparse
import struct
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

OUT = ROOT / "tests" / "golden" / "frag6"


def quirk_packets():
    import frag6_cases as f6

    return [(c.name, c.frag_size, c.id_base, c.linktype, c.batch().packet(0)) for c in f6.quirk_cases()]


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
            for _, fs, ident, link, p in cases:
                f.write(struct.pack("<IIII", fs, ident, link, len(p)) + p)
        print(len(cases), "cases written to", args.inputs)
    if args.recorded:
        raw = args.recorded.read_bytes()
        at = 4
        assert struct.unpack_from("<I", raw)[0] == len(cases)
        arrays = {}
        for name, fs, ident, link, p in cases:
            nfr, = struct.unpack_from("<I", raw, at)
            at += 4
            assert 1 <= nfr < 1000, name
            lens, body = [], b""
            for _ in range(nfr):
                ln, = struct.unpack_from("<I", raw, at)
                at += 4
                lens.append(ln)
                body += raw[at:at + ln]
                at += ln
            arrays[f"{name}.packet"] = np.frombuffer(p, np.uint8)
            arrays[f"{name}.rule"] = np.array([fs, ident, link], np.uint32)
            arrays[f"{name}.lens"] = np.array(lens, np.uint32)
            arrays[f"{name}.out"] = np.frombuffer(body, np.uint8)
            print(name, nfr, "fragments,", len(body), "bytes")
        assert at == len(raw)
        np.savez_compressed(OUT / "expected.npz", **arrays)


if __name__ == "__main__":
    main()
