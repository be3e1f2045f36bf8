"""Freeze the reference vectors of pcppx_tcpstream's tests (tests/golden/tcpstream/).

The reference's own TcpReassembly tests (Tests/Pcap++Test/Tests/TcpReassemblyTests.cpp) feed captures of
Tests/Pcap++Test/PcapExamples to TcpReassembly and compare what the callbacks deliver with text files beside them. This
tool copies those data files -- captures and expected streams; no program text is read or copied:

  python tools/make_golden_tcpstream.py <the reference's Tests/Pcap++Test/PcapExamples directory>
"""
from __future__ import annotations

import shutil
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
OUT = ROOT / "tests" / "golden" / "tcpstream"
FILES = (
    "three_http_streams.pcap", "three_http_streams_conn_1_output.txt", "three_http_streams_conn_2_output.txt",
    "three_http_streams_conn_3_output.txt", "one_http_stream_fin.pcap", "one_http_stream_fin_output.txt",
    "one_http_stream_fin2.pcap", "one_http_stream_fin2_output.txt", "one_tcp_stream.pcap", "one_tcp_stream_output.txt",
    "unidirectional_tcp_stream_with_missing_packet.pcap",
)


def main() -> None:
    if len(sys.argv) != 2 or not (Path(sys.argv[1]) / FILES[0]).exists():
        raise SystemExit(__doc__)
    OUT.mkdir(parents=True, exist_ok=True)
    for name in FILES:
        shutil.copyfile(Path(sys.argv[1]) / name, OUT / name)
        (OUT / name).chmod(0o644)
        print(name, (OUT / name).stat().st_size)


if __name__ == "__main__":
    main()
