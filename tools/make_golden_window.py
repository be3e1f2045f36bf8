"""Freeze the header-window grid (tests/window_cases.py) with the reference Packet++'s records (run where
oracle/_ref/libpcpp_ref.so is built, `make -C oracle ref`).

  python tools/make_golden_window.py

Writes tests/golden/window/grid.npz in the format of tools/make_golden.py: data, offsets, caplens, linktype, set_names
(the header kinds, "plain" last), set_index, and per option variant v: sum_<v>, lay_<v> (reference records), opts_<v>
(family, osi, csum, max_layers). The fixture holds packets and records only.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import oracle  # noqa: E402
import window_cases as wc  # noqa: E402
from pcapplusplus_amd import abi  # noqa: E402

OUT = ROOT / "tests" / "golden" / "window" / "grid.npz"
# parse-option variants pinned by the records: everything, Packet(&raw, TCP), and a shallow record (max_layers 5)
VARIANTS = {"full": (0, 8, 1, 16), "until_tcp": (4, 8, 1, 16), "ml5": (0, 8, 1, 5)}


def main() -> None:
    if not oracle.ref_available():
        raise SystemExit("oracle/_ref/libpcpp_ref.so missing: `make -C oracle ref` first")
    batch = wc.distinct_batch()
    names = list(wc.KINDS) + ["plain"]
    index = np.array([names.index(sl.kind) for sl in wc.grid()] + [len(names) - 1] * len(wc.PLAIN), np.int32)
    out = {"data": batch.data, "offsets": batch.offsets, "caplens": batch.caplens,
           "linktype": np.array(batch.linktype, np.int32), "set_names": np.array(names), "set_index": index}
    for v, (fam, osi, cs, ml) in VARIANTS.items():
        s, lay = oracle.ref_parse(batch, abi.make_opts(fam, osi, bool(cs), ml))
        out[f"sum_{v}"], out[f"lay_{v}"] = s, lay
        out[f"opts_{v}"] = np.array([fam, osi, cs, ml], np.int64)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT.name}: {batch.n} packets, {batch.data.nbytes} bytes -> {OUT.stat().st_size} B")


if __name__ == "__main__":
    main()
