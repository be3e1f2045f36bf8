"""Freeze the reference vectors of pcppx_ssl's tests (tests/golden/ssl/).

  python tools/make_golden_ssl.py <the reference's directory>

Copies data files only -- no program text is read or copied: the two expected reports of the reference's SSLAnalyzer
test (Tests/ExamplesTest/expected_output/sslanalyzer_tls.txt and sslanalyzer_manyprotocols.txt), tls.pcap whole, and
many_protocols_ssl.pcap: the packets of many-protocols.pcap, byte for byte and in file order, that are TCP with an SSL
port on either side (a superset of its SSL packets, so the report is unchanged) and every 16th other packet (thinned
further if the file would pass 1 MiB, never the SSL-port packets). packet_examples.pcap holds the Packet++Test SSL/TLS
packets in one capture. crafted.pcap holds the crafted packets of tests/ssl_cases.py and seeded byte mutations of the
captures' hello packets, cut behind the hello's record.

expected.npz (tests/test_ssl.py reads it) has one JSON text per capture: a list with one entry per packet, null where
the reference builds no SSL layer, else
  [the TCP layer's getLayerPayloadSize(), getSrcPort(), getDstPort(),
   [[getRecordType(), ClientHello or null, ServerHello or null], ... one per SSL layer]]
with a hello as [getHandshakeVersion(), getSessionIDLength(), getCipherSuiteCount() (client) or getCipherSuiteID()
(server), 1 (client) or its isValid (server), getExtensionCount(), the SNI getHostName() as hex or null, undefined].
undefined = 1 marks a hello the dump program must not ask the reference about, because the reference's answer is
undefined there: an SNI extension of length 1..4 (getHostName() is not called: the name is null) and a ServerHello
whose first extension of type 43 has length 0 (getHandshakeVersion() is not called: the version is 0).

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
OUT = ROOT / "tests" / "golden" / "ssl"
REF_SO_DIR = ROOT / "oracle" / "_ref"
EXAMPLES_TEST = "Tests/ExamplesTest"
PACKET_EXAMPLES = "Tests/Packet++Test/PacketExamples"
REPORTS = ("sslanalyzer_tls.txt", "sslanalyzer_manyprotocols.txt")
EXTRA = ("tls1_3.pcap", "tls_grease.pcap", "tls_server_hello.pcap", "tls_zero_size_ext.pcap", "ssl-malformed1.pcap")
LIMIT = 1 << 20
MUTATED, SEED, BUDGET = 2000, 20261021, 900_000  # mutations, as many as keep crafted.pcap under 1 MiB

DUMP = r"""
#include <cstdio>
#include <string>
#include "Packet.h"
#include "PcapFileDevice.h"
#include "SSLLayer.h"
#include "TcpLayer.h"
using namespace pcpp;
static void client(SSLClientHelloMessage* m) {
  SSLExtension* sni = m->getExtensionOfType((uint16_t)0);
  const bool undef = sni != nullptr && sni->getLength() >= 1 && sni->getLength() < 5;
  std::printf("[%u,%u,%d,1,%d,", (unsigned)m->getHandshakeVersion().asUInt(), (unsigned)m->getSessionIDLength(),
              m->getCipherSuiteCount(), m->getExtensionCount());
  SSLServerNameIndicationExtension* ext = m->getExtensionOfType<SSLServerNameIndicationExtension>();
  if (ext == nullptr || undef) {
    std::printf("null");
  } else {
    std::printf("\"");
    for (unsigned char c : ext->getHostName()) std::printf("%02x", c);
    std::printf("\"");
  }
  std::printf(",%d]", undef ? 1 : 0);
}
static void server(SSLServerHelloMessage* m) {
  SSLExtension* sv = nullptr;  // by index: the ServerHello's lookup by number compares the enum, which lacks 43
  for (int i = 0; sv == nullptr && i < m->getExtensionCount(); ++i)
    if (m->getExtension(i)->getTypeAsInt() == 43) sv = m->getExtension(i);
  const bool undef = sv != nullptr && sv->getLength() == 0;
  bool valid = false;
  const unsigned id = m->getCipherSuiteID(valid);
  std::printf("[%u,%u,%u,%d,%d,null,%d]", undef ? 0u : (unsigned)m->getHandshakeVersion().asUInt(),
              (unsigned)m->getSessionIDLength(), id, valid ? 1 : 0, m->getExtensionCount(), undef ? 1 : 0);
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
    SSLLayer* ssl = packet.getLayerOfType<SSLLayer>();
    TcpLayer* tcp = packet.getLayerOfType<TcpLayer>();
    if (ssl == nullptr || tcp == nullptr) { std::printf("null"); continue; }
    std::printf("[%zu,%u,%u,[", tcp->getLayerPayloadSize(), (unsigned)tcp->getSrcPort(), (unsigned)tcp->getDstPort());
    const char* sep = "";
    for (; ssl != nullptr; ssl = packet.getNextLayerOfType<SSLLayer>(ssl)) {
      std::printf("%s[%d,", sep, (int)ssl->getRecordType());
      sep = ",";
      SSLHandshakeLayer* hs = dynamic_cast<SSLHandshakeLayer*>(ssl);
      SSLClientHelloMessage* ch = hs != nullptr ? hs->getHandshakeMessageOfType<SSLClientHelloMessage>() : nullptr;
      SSLServerHelloMessage* sh = hs != nullptr ? hs->getHandshakeMessageOfType<SSLServerHelloMessage>() : nullptr;
      if (ch != nullptr) client(ch); else std::printf("null");
      std::printf(",");
      if (sh != nullptr) server(sh); else std::printf("null");
      std::printf("]");
    }
    std::printf("]]");
  }
  std::printf("\n]\n");
  return 0;
}
"""


def build_dump(ref: Path, tmp: Path) -> Path:
    src, exe = tmp / "ssl_dump.cpp", tmp / "ssl_dump"
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


def ssl_port_subset(capture):
    """Every TCP packet with an SSL port on either side, and every `step`th other packet, in file order."""
    from pcapplusplus_amd import ssl as sl

    summary, layers = parse(capture)
    on_port = np.zeros(capture.n, bool)
    for i in range(capture.n):
        pk = capture.packet(i)
        for e in layers[i][:int(summary["n_layers"][i])]:
            o = int(e["offset"])
            if int(e["proto"]) == sl.P_TCP and o + 4 <= len(pk):
                on_port[i] |= int.from_bytes(pk[o:o + 2], "big") in sl.SSL_PORTS or \
                    int.from_bytes(pk[o + 2:o + 4], "big") in sl.SSL_PORTS
    others = np.nonzero(~on_port)[0]
    step = 16
    while True:
        keep = np.sort(np.concatenate([np.nonzero(on_port)[0], others[::step]]))
        size = 24 + int((capture.caplens[keep].astype(np.int64) + 16).sum())
        if size < LIMIT:
            return subset(capture, keep), int(on_port.sum()), step
        step *= 2


def hello_packets(capture) -> list[tuple[int, int, int]]:
    """(packet, the record's first byte, its end) of the packets whose first SSL entry is a handshake record that
    starts with a hello."""
    summary, layers = parse(capture)
    out = []
    for i in range(capture.n):
        pk = capture.packet(i)
        for e in layers[i][:int(summary["n_layers"][i])]:
            o = int(e["offset"])
            if int(e["proto"]) == 18:
                if pk[o] == 22 and o + 6 <= len(pk) and pk[o + 5] in (1, 2):
                    out.append((i, o, o + int(e["hdr_len"])))
                break
    return out


def crafted_packets(captures: list) -> list[bytes]:
    """The crafted set: tests/ssl_cases.py's branches and seeded mutations, then seeded byte mutations of the
    captures' hello packets, each cut behind the hello's record (a third of them inside it)."""
    import ssl_cases as sc

    out = sc.record_types() + sc.hello_cases() + sc.later_entries() + sc.many_records() + sc.fuzz(300, SEED)
    size = sum(len(p) + 16 for p in out)
    pool = [(c, i, at, end) for c in captures for i, at, end in hello_packets(c)]
    rng = np.random.default_rng(SEED + 1)
    for _ in range(MUTATED):
        c, i, at, end = pool[int(rng.integers(len(pool)))]
        pkt = bytearray(c.packet(i)[:end])
        for _ in range(int(rng.integers(1, 5))):
            j = at + int(rng.integers(len(pkt) - at))
            kind = int(rng.integers(3))
            pkt[j] = int(rng.integers(256)) if kind == 0 else pkt[j] ^ (1 << int(rng.integers(8))) if kind == 1 \
                else int(rng.integers(6))
        if rng.integers(3) == 0:
            pkt = pkt[:int(rng.integers(at + 6, len(pkt) + 1))]
        if pkt[12:14] == b"\x08\x00":
            pkt[16:18] = (len(pkt) - 14).to_bytes(2, "big")  # the IPv4 total length follows the cut
        if size + len(pkt) + 16 > BUDGET:
            break
        size += len(pkt) + 16
        out.append(bytes(pkt))
    return out


def save_frozen(path, frozen: dict) -> None:
    files = sorted(frozen)
    np.savez_compressed(path, files=np.array(files),
                        **{f"f{k}": np.frombuffer(json.dumps(frozen[f], separators=(",", ":")).encode(), np.uint8)
                           for k, f in enumerate(files)})


def main() -> None:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / EXAMPLES_TEST / "pcap_examples" / "tls.pcap").exists():
        raise SystemExit(__doc__)
    if not (REF_SO_DIR / "libpcpp_ref.so").exists():
        raise SystemExit("oracle/_ref/libpcpp_ref.so is missing: run build() where the reference's sources exist")
    from pcapplusplus_amd.pcap import concat, read_pcap, write_pcap

    ref = Path(sys.argv[1])
    OUT.mkdir(parents=True, exist_ok=True)
    copies = [(ref / EXAMPLES_TEST / "expected_output" / r, r) for r in REPORTS] + \
        [(ref / EXAMPLES_TEST / "pcap_examples" / "tls.pcap", "tls.pcap")]
    for src, name in copies:
        shutil.copyfile(src, OUT / name)
        (OUT / name).chmod(0o644)
        print(name, (OUT / name).stat().st_size)
    many, on_port, step = ssl_port_subset(read_pcap(ref / EXAMPLES_TEST / "pcap_examples" / "many-protocols.pcap"))
    write_pcap(OUT / "many_protocols_ssl.pcap", many)
    print("many_protocols_ssl.pcap", (OUT / "many_protocols_ssl.pcap").stat().st_size, many.n, "packets", on_port,
          "on an SSL port, every", step, "th of the others")
    examples = sorted((ref / PACKET_EXAMPLES).glob("SSL-*.pcap")) + [ref / PACKET_EXAMPLES / p for p in EXTRA]
    write_pcap(OUT / "packet_examples.pcap", concat([read_pcap(p) for p in examples]))
    print("packet_examples.pcap", (OUT / "packet_examples.pcap").stat().st_size)
    names = ["tls.pcap", "many_protocols_ssl.pcap", "packet_examples.pcap"]
    from pcapplusplus_amd.pcap import from_packets

    write_pcap(OUT / "crafted.pcap", from_packets(crafted_packets([read_pcap(OUT / n) for n in names])))
    print("crafted.pcap", (OUT / "crafted.pcap").stat().st_size)
    frozen = {}
    with tempfile.TemporaryDirectory() as d:
        exe = build_dump(ref, Path(d))
        for name in names + ["crafted.pcap"]:
            run = subprocess.run([str(exe), str(OUT / name)], check=True, capture_output=True, text=True)
            frozen[name] = json.loads(run.stdout)
            print(name, len(frozen[name]), "packets", sum(p is not None for p in frozen[name]), "with an SSL layer",
                  sum(1 for p in frozen[name] if p for l in p[3] for h in l[1:] if h and h[6]), "undefined hellos")
    save_frozen(OUT / "expected.npz", frozen)
    print("expected.npz", (OUT / "expected.npz").stat().st_size)
    for f in OUT.iterdir():
        assert f.stat().st_size < LIMIT, f


if __name__ == "__main__":
    main()
