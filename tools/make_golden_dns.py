"""Freeze the reference vectors of pcppx_dns's tests (tests/golden/dns/).

  python tools/make_golden_dns.py <the reference's Tests directory>

Copies data files only -- no program text is read or copied: Pcap++Test/PcapExamples/DnsPackets.pcap (464 packets),
the captures Dns.pcap and DnsEdit7.pcap and the hex packets Dns1-4, DnsTooManyResources, dns_stack_overflow and
dns_over_tcp_* of Packet++Test/PacketExamples. It writes crafted.pcap -- the crafted packets of tests/dns_cases.py
(every oddity of decodeName, every rule boundary, seeded mutations of crafted messages) and seeded byte mutations of
DnsPackets.pcap's messages -- and freezes resources.npz (tests/dns_cases.py has its layout): for every packet of these
files what the real DnsLayer links, per resource the section, getSize(), type, class, TTL, data length, data offset and
name bytes, and which packets the reference builds no DnsLayer in.

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
OUT = ROOT / "tests" / "golden" / "dns"
REF_SO_DIR = ROOT / "oracle" / "_ref"
CAPTURE = "Pcap++Test/PcapExamples/DnsPackets.pcap"
EXAMPLES = "Packet++Test/PacketExamples"
PCAPS = ("Dns.pcap", "DnsEdit7.pcap")
DATS = ("Dns1", "Dns2", "Dns3", "Dns4", "DnsTooManyResources", "dns_stack_overflow", "dns_over_tcp_answer",
        "dns_over_tcp_answer2", "dns_over_tcp_query", "dns_over_tcp_response")
MUTATED, SEED = 600, 20261020

DUMP = r"""
#include <cstdio>
#include <string>
#include "DnsLayer.h"
#include "Packet.h"
#include "PcapFileDevice.h"
using namespace pcpp;
static void name_hex(const std::string& s) {
  std::printf("\"");
  for (unsigned char c : s) std::printf("%02x", c);
  std::printf("\"");
}
static void query(const char* sep, DnsQuery* q) {
  std::printf("%s[0,%zu,%u,%u,0,0,0,", sep, q->getSize(), (unsigned)q->getDnsType(), (unsigned)q->getDnsClass());
  name_hex(q->getName());
  std::printf("]");
}
static void resource(const char* sep, int section, DnsResource* r) {
  std::printf("%s[%d,%zu,%u,%u,%u,%zu,%zu,", sep, section, r->getSize(), (unsigned)r->getDnsType(),
              (unsigned)r->getDnsClass(), (unsigned)r->getTTL(), r->getDataLength(), r->getDataOffset());
  name_hex(r->getName());
  std::printf("]");
}
int main(int argc, char** argv) {
  PcapFileReaderDevice reader(argv[1]);
  if (!reader.open()) return 2;
  RawPacket raw;
  std::printf("[");
  const char* psep = "";
  while (reader.getNextPacket(raw)) {
    Packet packet(&raw);
    DnsLayer* dns = packet.getLayerOfType<DnsLayer>();
    std::printf("%s\n", psep);
    psep = ",";
    if (dns == nullptr) { std::printf("null"); continue; }
    std::printf("[");
    const char* sep = "";
    for (DnsQuery* q = dns->getFirstQuery(); q != nullptr; q = dns->getNextQuery(q)) { query(sep, q); sep = ","; }
    for (DnsResource* r = dns->getFirstAnswer(); r != nullptr; r = dns->getNextAnswer(r)) { resource(sep, 1, r); sep = ","; }
    for (DnsResource* r = dns->getFirstAuthority(); r != nullptr; r = dns->getNextAuthority(r)) { resource(sep, 2, r); sep = ","; }
    for (DnsResource* r = dns->getFirstAdditionalRecord(); r != nullptr; r = dns->getNextAdditionalRecord(r)) { resource(sep, 3, r); sep = ","; }
    std::printf("]");
  }
  std::printf("\n]\n");
  return 0;
}
"""


def build_dump(ref: Path, tmp: Path) -> Path:
    src, exe = tmp / "dns_dump.cpp", tmp / "dns_dump"
    src.write_text(DUMP)
    inc = [f"-I{ref / p}" for p in ("Packet++/header", "Common++/header", "Pcap++/header",
                                    "3rdParty/EndianPortable/include")]
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", *inc, str(src), "-o", str(exe), f"-L{REF_SO_DIR}", "-lpcpp_ref",
                    f"-Wl,-rpath,{REF_SO_DIR}", "-pthread"], check=True)
    return exe


def crafted_packets(capture) -> list[bytes]:
    """The crafted set: tests/dns_cases.py's oddities, boundaries and seeded mutations, then seeded mutations of the
    capture's messages (the bytes of the DNS layer the parse's restatement records, from its fifth byte on)."""
    import dns_cases as dc
    import oracle
    from pcapplusplus_amd import abi

    out = dc.quirks() + dc.bounds() + dc.section_orders() + dc.fuzz(300, SEED)
    summary, layers = oracle.oracle_parse(capture, abi.make_opts())
    layers = np.ascontiguousarray(layers).reshape(capture.n, -1)
    rng = np.random.default_rng(SEED + 1)
    for _ in range(MUTATED):
        i = int(rng.integers(capture.n))
        at = [int(e["offset"]) for e in layers[i][:int(summary["n_layers"][i])] if int(e["proto"]) == 13]
        pkt = bytearray(capture.packet(i))
        dc.mutate(pkt, rng, at[0])
        out.append(bytes(pkt))
    return out


def main() -> None:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / CAPTURE).exists():
        raise SystemExit(__doc__)
    if not (REF_SO_DIR / "libpcpp_ref.so").exists():
        raise SystemExit("oracle/_ref/libpcpp_ref.so is missing: run build() where the reference's sources exist")
    from pcapplusplus_amd.pcap import from_packets, read_hex_dat, read_pcap, write_pcap

    tests = Path(sys.argv[1])
    ref = tests.parent
    OUT.mkdir(parents=True, exist_ok=True)
    copies = [(tests / CAPTURE, "DnsPackets.pcap")] + [(tests / EXAMPLES / p, p) for p in PCAPS] + \
        [(tests / EXAMPLES / f"{d}.dat", f"{d}.dat") for d in DATS]
    for src, name in copies:
        shutil.copyfile(src, OUT / name)
        (OUT / name).chmod(0o644)
        print(name, (OUT / name).stat().st_size)
    write_pcap(OUT / "crafted.pcap", from_packets(crafted_packets(read_pcap(OUT / "DnsPackets.pcap"))))
    print("crafted.pcap", (OUT / "crafted.pcap").stat().st_size)
    frozen = {}
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        exe = build_dump(ref, tmp)
        for name in ("DnsPackets.pcap", "crafted.pcap", *PCAPS, *[f"{x}.dat" for x in DATS]):
            path = OUT / name
            if name.endswith(".dat"):  # one Ethernet packet as hex text
                path = tmp / (name + ".pcap")
                write_pcap(path, from_packets([read_hex_dat(OUT / name)]))
            run = subprocess.run([str(exe), str(path)], check=True, capture_output=True, text=True)
            frozen[name] = json.loads(run.stdout)
            print(name, len(frozen[name]), "packets",
                  sum(len(p) for p in frozen[name] if p is not None), "resources")
    import dns_cases as dc

    dc.save_frozen(OUT / "resources.npz", frozen)
    print("resources.npz", (OUT / "resources.npz").stat().st_size)


if __name__ == "__main__":
    main()
