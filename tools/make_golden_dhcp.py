"""Freeze the reference vectors of pcppx_dhcp's tests (tests/golden/dhcp/).

  python tools/make_golden_dhcp.py <the reference's directory>

Copies data files only -- no program text is read or copied. packet_examples.pcap holds the Packet++Test DHCP packets
(Dhcp1..4.pcap, dhcpv6.pcap), the packets of example2.pcap and many-protocols.pcap with a UDP port 546 / 547, and every
16th other packet of the latter, in one Ethernet capture. crafted.pcap holds the crafted packets of
tests/dhcp_cases.py and seeded byte mutations of the real DHCP / DHCPv6 packets of packet_examples.pcap from the UDP
payload's first byte on; a third of them are cut short (DHCPv4 behind byte 230 of the payload, so that most of them
keep the 240 bytes a DhcpLayer needs; DHCPv6 anywhere in the payload), and the IPv4 / IPv6 and UDP lengths follow the
cut.

expected.npz (tests/test_dhcp.py reads it) has one JSON text per capture: a list with one entry per packet, null where
the reference builds no DhcpLayer / DhcpV6Layer, else
  [family (4 | 6), getDataLen(), getMessageType(), getOptionsCount() / getOptionCount(),
   DHCPv4: [getOpCode(), getClientIpAddress(), getYourIpAddress(), getServerIpAddress(), getGatewayIpAddress() and
            getClientHardwareAddress() as hex, the header's xid, secs and flags in host order];
   DHCPv6: [getTransactionID()],
   [[type, getDataSize(), value as hex], ... every option of getFirstOptionData() / getNextOptionData()]]
A DHCPv6 option's type is the record's first two bytes, big-endian (getType() folds the codes outside its enum to 0).

The tool asserts when it freezes: every file is under 1 MiB; in crafted.pcap at least half of the packets carry a DHCP
or DHCPv6 layer by the reference; each family has at least 100 such packets.

The records come from a small dump program (its text is below) compiled into a temporary directory against the
reference's headers and oracle/_ref/libpcpp_ref.so (build() makes it where the reference's sources exist); nothing
compiled is kept. The tool runs only where those exist; the tests read only the frozen data.
"""
from __future__ import annotations

import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "dhcp"
REF_SO_DIR = ROOT / "oracle" / "_ref"
PACKET_EXAMPLES = "Tests/Packet++Test/PacketExamples"
EXAMPLE2 = "Tests/Pcap++Test/PcapExamples/example2.pcap"
MANY = "Tests/ExamplesTest/pcap_examples/many-protocols.pcap"
LIMIT = 1 << 20
MUTATED, SEED, BUDGET = 1500, 20261021, 960_000  # mutations, as many as keep crafted.pcap under 1 MiB
V4_CUT_FROM = 230                                # a cut DHCPv4 payload keeps at least this many bytes

DUMP = r"""
#include <cstdio>
#include <cstring>
#include "Packet.h"
#include "PcapFileDevice.h"
#include "DhcpLayer.h"
#include "DhcpV6Layer.h"
#include "EndianPortable.h"
using namespace pcpp;
static void hex(const uint8_t* p, size_t n) {
  std::printf("\"");
  for (size_t k = 0; k < n; ++k) std::printf("%02x", p[k]);
  std::printf("\"");
}
static void ip(const IPv4Address& a) { hex(a.toBytes(), 4); }
int main(int argc, char** argv) {
  IFileReaderDevice* reader = IFileReaderDevice::getReader(argv[1]);
  if (reader == nullptr || !reader->open()) return 2;
  RawPacket raw;
  std::printf("[");
  const char* psep = "";
  while (reader->getNextPacket(raw)) {
    std::printf("%s\n", psep);
    psep = ",";
    Packet packet(&raw);
    DhcpLayer* d4 = packet.getLayerOfType<DhcpLayer>();
    DhcpV6Layer* d6 = packet.getLayerOfType<DhcpV6Layer>();
    if (d4 != nullptr) {
      dhcp_header* h = d4->getDhcpHeader();
      std::printf("[4,%zu,%d,%zu,[%d,", d4->getDataLen(), (int)d4->getMessageType(), d4->getOptionsCount(),
                  (int)d4->getOpCode());
      ip(d4->getClientIpAddress()); std::printf(",");
      ip(d4->getYourIpAddress()); std::printf(",");
      ip(d4->getServerIpAddress()); std::printf(",");
      ip(d4->getGatewayIpAddress()); std::printf(",");
      hex(d4->getClientHardwareAddress().getRawData(), 6);
      std::printf(",%u,%u,%u],[", (unsigned)be32toh(h->transactionID), (unsigned)be16toh(h->secondsElapsed),
                  (unsigned)be16toh(h->flags));
      const char* sep = "";
      for (DhcpOption o = d4->getFirstOptionData(); o.isNotNull(); o = d4->getNextOptionData(o)) {
        std::printf("%s[%u,%zu,", sep, (unsigned)o.getType(), o.getDataSize());
        sep = ",";
        hex(o.getValue(), o.getDataSize());
        std::printf("]");
      }
      std::printf("]]");
    } else if (d6 != nullptr) {
      std::printf("[6,%zu,%d,%zu,[%u],[", d6->getDataLen(), (int)d6->getMessageType(), d6->getOptionCount(),
                  (unsigned)d6->getTransactionID());
      const char* sep = "";
      for (DhcpV6Option o = d6->getFirstOptionData(); o.isNotNull(); o = d6->getNextOptionData(o)) {
        const uint8_t* p = o.getRecordBasePtr();
        std::printf("%s[%u,%zu,", sep, (unsigned)p[0] << 8 | p[1], o.getDataSize());
        sep = ",";
        hex(o.getValue(), o.getDataSize());
        std::printf("]");
      }
      std::printf("]]");
    } else {
      std::printf("null");
    }
  }
  std::printf("\n]\n");
  return 0;
}
"""


def build_dump(ref: Path, tmp: Path) -> Path:
    src, exe = tmp / "dhcp_dump.cpp", tmp / "dhcp_dump"
    src.write_text(DUMP)
    inc = [f"-I{ref / p}" for p in ("Packet++/header", "Common++/header", "Pcap++/header",
                                    "3rdParty/EndianPortable/include")]
    subprocess.run(["g++", "-O1", "-std=c++17", "-w", *inc, str(src), "-o", str(exe), f"-L{REF_SO_DIR}", "-lpcpp_ref",
                    f"-Wl,-rpath,{REF_SO_DIR}", "-pthread"], check=True)
    return exe


def parse(capture):
    import oracle
    from pcapplusplus_amd import abi

    summary, layers = oracle.oracle_parse(capture, abi.make_opts())
    return summary, np.ascontiguousarray(layers).reshape(capture.n, -1)


def subset(capture, keep) -> "PacketBatch":  # noqa: F821
    from pcapplusplus_amd.pcap import PacketBatch

    cut = lambda a: None if a is None else a[keep]  # noqa: E731
    return PacketBatch(capture.data, capture.offsets[keep], capture.caplens[keep], capture.linktype,
                       cut(capture.timestamps_ns), cut(capture.frame_lens))


def v6_candidates(capture) -> np.ndarray:
    """Per packet: a UDP entry of its chain has a port 546 / 547."""
    from pcapplusplus_amd import dhcp as dh

    summary, layers = parse(capture)
    out = np.zeros(capture.n, bool)
    for i in range(capture.n):
        pk = capture.packet(i)
        for e in layers[i][:int(summary["n_layers"][i])]:
            o = int(e["offset"])
            if int(e["proto"]) == dh.P_UDP and o + 4 <= len(pk):
                out[i] |= bool({int.from_bytes(pk[o:o + 2], "big"), int.from_bytes(pk[o + 2:o + 4], "big")} & {546, 547})
    return out


def with_others(capture, step: int):
    """Every port-546/547 packet, and with step every step-th other packet, in file order."""
    cand = v6_candidates(capture)
    others = np.nonzero(~cand)[0]
    keep = np.sort(np.concatenate([np.nonzero(cand)[0], others[::step] if step else others[:0]]))
    return subset(capture, keep), int(cand.sum())


def dhcp_packets(capture) -> list[tuple[int, int, int]]:
    """(packet, the payload's first byte, family) of the packets the contract finds a message in, by its Python
    model."""
    from pcapplusplus_amd import abi
    from pcapplusplus_amd import dhcp as dh

    summary, layers = parse(capture)
    out = []
    for i in range(capture.n):
        lay = dh.find_layer(capture.packet(i), layers[i], int(summary["n_layers"][i]), abi.make_opts().max_layers,
                            int(summary["flags"][i]))
        if lay is not None and lay != dh.HOST:
            out.append((i, lay[0], lay[2]))
    return out


def crafted_packets(capture) -> list[bytes]:
    """The crafted set of tests/dhcp_cases.py, then seeded byte mutations of the capture's DHCP / DHCPv6 packets."""
    import dhcp_cases as dc
    from sip_cases import MUTATION_BYTES

    out = dc.crafted_packets()
    size = sum(len(p) + 16 for p in out)
    pool = dhcp_packets(capture)
    rng = np.random.default_rng(SEED)
    for _ in range(MUTATED):
        i, at, family = pool[int(rng.integers(len(pool)))]
        pkt = bytearray(capture.packet(i))
        for _ in range(int(rng.integers(1, 5))):
            j = at + int(rng.integers(len(pkt) - at))
            kind = int(rng.integers(3))
            pkt[j] = int(rng.integers(256)) if kind == 0 else pkt[j] ^ (1 << int(rng.integers(8))) if kind == 1 \
                else MUTATION_BYTES[int(rng.integers(len(MUTATION_BYTES)))]
        if rng.integers(3) == 0:
            low = at + (V4_CUT_FROM if family == 4 else 1)
            pkt = pkt[:int(rng.integers(min(low, len(pkt)), len(pkt) + 1))]
            if pkt[12:14] == b"\x08\x00" and at == 14 + 4 * (pkt[14] & 15) + 8:
                pkt[16:18] = (len(pkt) - 14).to_bytes(2, "big")            # the IPv4 total length follows the cut
                pkt[at - 4:at - 2] = (len(pkt) - at + 8).to_bytes(2, "big")  # and the UDP length
            elif pkt[12:14] == b"\x86\xdd" and at == 62:
                pkt[18:20] = (len(pkt) - 54).to_bytes(2, "big")            # the IPv6 payload length
                pkt[at - 4:at - 2] = (len(pkt) - at + 8).to_bytes(2, "big")
        if size + len(pkt) + 16 > BUDGET:
            break
        size += len(pkt) + 16
        out.append(bytes(pkt))
    return out


def main() -> None:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / PACKET_EXAMPLES / "Dhcp1.pcap").exists():
        raise SystemExit(__doc__)
    if not (REF_SO_DIR / "libpcpp_ref.so").exists():
        raise SystemExit("oracle/_ref/libpcpp_ref.so is missing: run build() where the reference's sources exist")
    import dhcp_cases as dc
    from pcapplusplus_amd import abi
    from pcapplusplus_amd.pcap import concat, from_packets, read_pcap, write_pcap

    ref = Path(sys.argv[1])
    OUT.mkdir(parents=True, exist_ok=True)
    parts = [read_pcap(ref / PACKET_EXAMPLES / f"{n}.pcap") for n in ("Dhcp1", "Dhcp2", "Dhcp3", "Dhcp4", "dhcpv6")]
    ex2, n2 = with_others(read_pcap(ref / EXAMPLE2), 0)
    many, nm = with_others(read_pcap(ref / MANY), 16)
    parts += [ex2, many]
    assert all(p.linktype == abi.LINKTYPE_ETHERNET for p in parts)
    write_pcap(OUT / "packet_examples.pcap", concat(parts))
    print("packet_examples.pcap", sum(p.n for p in parts), "packets;", n2, "and", nm, "with a port 546 / 547")
    write_pcap(OUT / "crafted.pcap", from_packets(crafted_packets(read_pcap(OUT / "packet_examples.pcap"))))
    frozen = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_dump(ref, Path(d))
        for name in ("packet_examples.pcap", "crafted.pcap"):
            run = subprocess.run([str(exe), str(OUT / name)], check=True, capture_output=True, text=True)
            ps = frozen[name] = json.loads(run.stdout)
            v4 = sum(isinstance(p, list) and p[0] == 4 for p in ps)
            v6 = sum(isinstance(p, list) and p[0] == 6 for p in ps)
            print(name, (OUT / name).stat().st_size, "bytes", len(ps), "packets", v4, "with a DHCP layer", v6,
                  "with a DHCPv6 layer")
            if name == "crafted.pcap":
                assert 2 * (v4 + v6) >= len(ps) and v4 >= 100 and v6 >= 100, (len(ps), v4, v6)
    dc.save_frozen(OUT / "expected.npz", frozen)
    print("expected.npz", (OUT / "expected.npz").stat().st_size, "bytes")
    for f in OUT.iterdir():
        assert f.stat().st_size < LIMIT, f


if __name__ == "__main__":
    main()
