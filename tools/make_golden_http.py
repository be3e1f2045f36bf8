"""Freeze the reference vectors of pcppx_http's tests (tests/golden/http/).

  python tools/make_golden_http.py <the reference's Tests directory>

Copies data files only -- no program text is read or copied: Pcap++Test/PcapExamples/4KHttpRequests.pcap and
650HttpResponses.pcap, ExamplesTest/pcap_examples/http-packets2.pcap and the captures TwoHttpRequests.pcap,
TwoHttpResponses.pcap, PartialHttpRequest.pcap and HttpMalformedResponse.pcapng of Packet++Test/PacketExamples. It
writes crafted.pcap -- the crafted packets of tests/http_cases.py (every branch of the first lines, of a field and of the
walk, the content lengths, seeded mutations of them) and seeded byte mutations and truncations of the captures' HTTP
packets -- and freezes fields.npz (tests/http_cases.py has its layout): for every packet of these files what the real
HttpRequestLayer / HttpResponseLayer reports -- the header length, the field count, the first line, the content length,
every field's name, value and size and which field getFieldByName returns -- and which packets the reference builds no
HTTP layer in.

The records come from a small dump program (its text is below) compiled into a temporary directory against the
reference's headers and oracle/_ref/libpcpp_ref.so (build() makes it where the reference's sources exist); nothing
compiled is kept. The tool runs only where those exist; the tests read only the frozen data.
"""
from __future__ import annotations

import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "http"
REF_SO_DIR = ROOT / "oracle" / "_ref"
CAPTURES = ("Pcap++Test/PcapExamples/4KHttpRequests.pcap", "Pcap++Test/PcapExamples/650HttpResponses.pcap",
            "ExamplesTest/pcap_examples/http-packets2.pcap")
HTTP_PACKETS = (385, 682, 115)  # the packets of CAPTURES in which the real reference builds an HTTP layer
EXAMPLES = "Packet++Test/PacketExamples"
SMALL = ("TwoHttpRequests.pcap", "TwoHttpResponses.pcap", "PartialHttpRequest.pcap", "HttpMalformedResponse.pcapng")
MUTATED, SEED = 1200, 20261020  # as many as keep crafted.pcap under 1 MiB

DUMP = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include "HttpLayer.h"
#include "Packet.h"
#include "PcapFileDevice.h"
using namespace pcpp;
static void hex(const std::string& s) {
  std::printf("\"");
  for (unsigned char c : s) std::printf("%02x", c);
  std::printf("\"");
}
static void fields(HttpMessage* m) {
  std::printf("[");
  const char* sep = "";
  for (HeaderField* f = m->getFirstField(); f != nullptr; f = m->getNextField(f)) {
    std::printf("%s[", sep);
    sep = ",";
    hex(f->getFieldName());
    std::printf(",");
    hex(f->getFieldValue());
    std::printf(",%zu,%d,%d]", f->getFieldSize(), f->isEndOfHeader() ? 1 : 0,
                !f->isEndOfHeader() && m->getFieldByName(f->getFieldName()) == f ? 1 : 0);
  }
  std::printf("]");
}
int main(int argc, char** argv) {
  IFileReaderDevice* reader = IFileReaderDevice::getReader(argv[1]);
  if (reader == nullptr || !reader->open()) return 2;
  RawPacket raw;
  std::printf("[");
  const char* psep = "";
  while (reader->getNextPacket(raw)) {
    Packet packet(&raw);
    std::printf("%s\n", psep);
    psep = ",";
    Layer* l = packet.getFirstLayer();
    while (l != nullptr && l->getProtocol() != HTTPRequest && l->getProtocol() != HTTPResponse) l = l->getNextLayer();
    if (l == nullptr) { std::printf("null"); continue; }
    HttpMessage* m = static_cast<HttpMessage*>(l);
    HeaderField* cl = m->getFieldByName("content-length");
    const int length = cl != nullptr ? std::atoi(cl->getFieldValue().c_str()) : 0;
    if (l->getProtocol() == HTTPRequest) {
      HttpRequestLayer* q = static_cast<HttpRequestLayer*>(l);
      HttpRequestFirstLine* f = q->getFirstLine();
      std::printf("[0,%zu,%d,%d,%d,%d,%d,", q->getHeaderLen(), q->getFieldCount(), q->isHeaderComplete() ? 1 : 0,
                  f->getSize(), (int)f->getMethod(), (int)f->getVersion());
      hex(f->getUri());
      std::printf(",0,%d,%d,%d,", f->isComplete() ? 1 : 0, length, cl != nullptr ? 1 : 0);
    } else {
      HttpResponseLayer* r = static_cast<HttpResponseLayer*>(l);
      HttpResponseFirstLine* f = r->getFirstLine();
      std::printf("[1,%zu,%d,%d,%d,9,%d,", r->getHeaderLen(), r->getFieldCount(), r->isHeaderComplete() ? 1 : 0,
                  f->getSize(), (int)f->getVersion());
      hex(f->getStatusCodeString());
      std::printf(",%d,%d,%d,%d,", f->getStatusCodeAsInt(), f->isComplete() ? 1 : 0, r->getContentLength(),
                  cl != nullptr ? 1 : 0);
    }
    fields(m);
    std::printf("]");
  }
  std::printf("\n]\n");
  return 0;
}
"""


def build_dump(ref: Path, tmp: Path) -> Path:
    src, exe = tmp / "http_dump.cpp", tmp / "http_dump"
    src.write_text(DUMP)
    inc = [f"-I{ref / p}" for p in ("Packet++/header", "Common++/header", "Pcap++/header",
                                    "3rdParty/EndianPortable/include")]
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", *inc, str(src), "-o", str(exe), f"-L{REF_SO_DIR}", "-lpcpp_ref",
                    f"-Wl,-rpath,{REF_SO_DIR}", "-pthread"], check=True)
    return exe


def http_packets(capture) -> list[tuple[int, int]]:
    """(packet, the HTTP layer's first byte) of the packets the parse's restatement records an HTTP layer in."""
    import oracle
    from pcapplusplus_amd import abi

    summary, layers = oracle.oracle_parse(capture, abi.make_opts())
    layers = np.ascontiguousarray(layers).reshape(capture.n, -1)
    out = []
    for i in range(capture.n):
        at = [int(e["offset"]) for e in layers[i][:int(summary["n_layers"][i])] if int(e["proto"]) in (6, 7)]
        if at:
            out.append((i, at[0]))
    return out


def crafted_packets(captures: list) -> list[bytes]:
    """The crafted set: tests/http_cases.py's branches and seeded mutations, then seeded mutations and truncations of
    the captures' HTTP packets."""
    import http_cases as hc

    out = hc.lines() + hc.header_cases() + hc.content_lengths() + hc.fuzz(300, SEED)
    pool = [(c, i, at) for c in captures for i, at in http_packets(c)]
    rng = np.random.default_rng(SEED + 1)
    for _ in range(MUTATED):
        c, i, at = pool[int(rng.integers(len(pool)))]
        pkt = bytearray(c.packet(i))
        hc.mutate(pkt, rng, at)
        if rng.integers(3) == 0 and len(pkt) > at + 1:
            pkt = pkt[:int(rng.integers(at + 1, len(pkt) + 1))]
            pkt[16:18] = (len(pkt) - 14).to_bytes(2, "big")  # the IPv4 total length follows the cut
        out.append(bytes(pkt))
    return out


def main() -> None:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / CAPTURES[0]).exists():
        raise SystemExit(__doc__)
    if not (REF_SO_DIR / "libpcpp_ref.so").exists():
        raise SystemExit("oracle/_ref/libpcpp_ref.so is missing: run build() where the reference's sources exist")
    from pcapplusplus_amd.pcap import from_packets, read_pcap, write_pcap

    tests = Path(sys.argv[1])
    ref = tests.parent
    OUT.mkdir(parents=True, exist_ok=True)
    copies = [(tests / c, Path(c).name) for c in CAPTURES] + [(tests / EXAMPLES / p, p) for p in SMALL]
    for src, name in copies:
        shutil.copyfile(src, OUT / name)
        (OUT / name).chmod(0o644)
        print(name, (OUT / name).stat().st_size)
    captures = [read_pcap(OUT / Path(c).name) for c in CAPTURES]
    write_pcap(OUT / "crafted.pcap", from_packets(crafted_packets(captures)))
    print("crafted.pcap", (OUT / "crafted.pcap").stat().st_size)
    frozen = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_dump(ref, Path(d))
        for name in [Path(c).name for c in CAPTURES] + list(SMALL) + ["crafted.pcap"]:
            run = subprocess.run([str(exe), str(OUT / name)], check=True, capture_output=True, text=True)
            frozen[name] = json.loads(run.stdout)
            print(name, len(frozen[name]), "packets", sum(p is not None for p in frozen[name]), "with an HTTP layer")
    for c, want in zip(CAPTURES, HTTP_PACKETS):
        got = sum(p is not None for p in frozen[Path(c).name])
        assert got == want, (c, got, want)
    import http_cases as hc

    hc.save_frozen(OUT / "fields.npz", frozen)
    print("fields.npz", (OUT / "fields.npz").stat().st_size)


if __name__ == "__main__":
    main()
