"""SSL/TLS records and hellos in plain Python: builders, the independent model of the ssl contract, the per-hello rows
and SSLAnalyzer's tables.

SSLLayer builds one layer per TLS record, SSLHandshakeLayer one message object per handshake message
(Packet++/src/SSLLayer.cpp:42-150, SSLHandshake.cpp:1287-1350), and Examples/SSLAnalyzer reads the record types, the
hellos, the ServerHello's version and cipher suite and the ClientHello's SNI host name of every packet
(SSLStatsCollector.h:141-401). pcppx_ssl_device / pcppx_ssl_reference produce one record per SSL packet and per hello
(include/pcppx.h, ssl). This module holds

  record() / handshake() / client_hello() / server_hello() / extension() / sni() / tcp_packet()
             crafted records, messages and packets for the tests and the benchmark,
  model()    the ssl contract restated packet by packet over Python byte strings and slices: it shares no code with
             the C++ / HIP implementation and is what the tests compare pcppx_ssl_reference with,
  rows()     messages, hello records and names turned into one row per hello record,
  analyze()  SSLAnalyzer's tables from the records of a call with kinds 3 and the parse's hash5 column.
"""
from __future__ import annotations

import struct
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .http import tcp_packet as _tcp_packet

P_SSL, P_TCP = 18, 4  # pcpp::SSL, pcpp::TCP
CCS, ALERT, HANDSHAKE, APPDATA = 20, 21, 22, 23
SSL_PORTS = (443, 261, 448, 465, 563, 614, 636, 989, 990, 992, 993, 994, 995)  # SSLLayer::isSSLPort
KNOWN_TYPES = (0, 1, 2, 4, 11, 12, 13, 14, 15, 16, 20)  # the cases of createHandshakeMessage's switch


# ------------------------------------------------------------------ builders
def record(kind: int, body: bytes, version: int = 0x0303, length: int | None = None) -> bytes:
    """A TLS record: type, version, length (None: the body's) and the body."""
    return struct.pack(">BHH", kind, version, len(body) if length is None else length) + body


def handshake(kind: int, body: bytes, length: int | None = None, length1: int = 0) -> bytes:
    """A handshake message: type, the 24-bit length as its top byte and low word, the body."""
    return struct.pack(">BBH", kind, length1, (len(body) if length is None else length) & 0xFFFF) + body


def extension(kind: int, data: bytes = b"", length: int | None = None) -> bytes:
    return struct.pack(">HH", kind, len(data) if length is None else length) + data


def sni(name: bytes, name_len: int | None = None, list_len: int | None = None) -> bytes:
    """A server-name extension: list length, name type 0, name length (None: the name's), the name."""
    nl = len(name) if name_len is None else name_len
    return extension(0, struct.pack(">HBH", nl + 3 if list_len is None else list_len, 0, nl) + name)


def _ext_block(extensions, ext_len: int | None) -> bytes:
    if extensions is None:
        return b""
    raw = b"".join(extensions)
    return struct.pack(">H", len(raw) if ext_len is None else ext_len) + raw


def client_hello(extensions=(), ciphers=(0x1301, 0xC02F, 0x002F), sid: bytes = b"", version: int = 0x0303,
                 ext_len: int | None = None, length: int | None = None) -> bytes:
    """A ClientHello message; extensions: raw extension() byte strings, or None for no extension block at all."""
    body = struct.pack(">H", version) + bytes(range(32)) + bytes([len(sid)]) + sid + \
        struct.pack(">H", 2 * len(ciphers)) + b"".join(struct.pack(">H", c) for c in ciphers) + b"\x01\x00" + \
        _ext_block(extensions, ext_len)
    return handshake(1, body, length)


def server_hello(extensions=(), cipher: int = 0xC02F, sid: bytes = b"", version: int = 0x0303,
                 ext_len: int | None = None, length: int | None = None) -> bytes:
    body = struct.pack(">H", version) + bytes(range(32)) + bytes([len(sid)]) + sid + struct.pack(">HB", cipher, 0) + \
        _ext_block(extensions, ext_len)
    return handshake(2, body, length)


def tcp_packet(payload: bytes, k: int = 0, from_server: bool = False, port: int = 443) -> bytes:
    """Ethernet / IPv4 / TCP around a payload on an SSL port; the payload starts at byte 54."""
    return _tcp_packet(payload, k, from_server, port)


# ------------------------------------------------------------------ the contract (include/pcppx.h, ssl), restated
def incomplete_chain(flags: int, n_layers: int, max_layers: int) -> bool:
    """Rule 2."""
    if flags & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW):
        return True
    if n_layers > max_layers:
        return True
    return bool(flags & abi.F_NEEDS_HOST_L7) and (bool(flags & abi.F_L7_SSL) or not flags & abi.F_L7_KNOWN)


def _be16(d: bytes, at: int) -> int:
    return int.from_bytes(d[at:at + 2], "big")


def extensions_of(m: bytes, E: int, M: int) -> list[tuple]:
    """tlsfp's rule 5 over a message's D readable bytes m: (type, data position, length) of every listed extension."""
    D = len(m)
    if E + 2 > D:
        return []
    it = E + 2
    end = min(it + _be16(m, E), M)
    out = []
    while end - it >= 4:
        kind, ln = _be16(m, it), _be16(m, it + 2)
        if end - it < 4 + ln:
            break
        out.append((kind, it + 4, ln))
        it += 4 + ln
    return out


@dataclass
class Hello:
    kind: int
    layer: int
    msg_offset: int
    name: bytes = b""
    version: int = 0
    header_version: int = 0
    cipher: int = 0
    n_ciphers: int = 0
    n_ext: int = 0
    sid: int = 0
    flags: int = 0


def hello_of(m: bytes, M: int, kind: int, layer: int, msg_offset: int) -> Hello:
    """Rules 5-7 over the D bytes m from the message's first byte to the record's end."""
    D = len(m)
    h = Hello(kind, layer, msg_offset)
    h.sid = 0 if D <= 39 else min(m[38], D - 39)
    h.header_version = h.version = 0 if D < 6 else _be16(m, 4)
    cs = 39 + h.sid
    if kind == abi.SSL_CLIENT:
        h.n_ciphers = 0 if cs + 2 > D else _be16(m, cs) // 2
        exts = extensions_of(m, cs + 2 + 2 * h.n_ciphers + 2, M)
        names = [e for e in exts if e[0] == 0]
        if names:
            _, x, L = names[0]
            h.flags |= abi.SSL_HAS_SNI
            if L >= 5:
                want = _be16(m, x + 3)
                h.name = m[x + 5:min(x + 5 + want, x + L)]
                if x + 5 + want > x + L:
                    h.flags |= abi.SSL_SNI_TRUNCATED
            elif L >= 1:
                h.flags |= abi.SSL_SNI_MALFORMED
    else:
        if cs + 2 <= D:
            h.cipher = _be16(m, cs)
            h.flags |= abi.SSL_HAS_CIPHER
        exts = extensions_of(m, cs + 3, M)
        versions = [e for e in exts if e[0] == 43]
        if versions:
            _, x, L = versions[0]
            if L == 2:
                h.version = _be16(m, x)
            elif L == 3 and m[x] == 2:
                h.version = _be16(m, x + 1)
    h.n_ext = len(exts)
    return h


def handshake_hellos(rec: bytes, layer: int, offset: int) -> list[Hello]:
    """Rule 4 over a handshake entry's R bytes behind its 5-byte header: its first ClientHello and first ServerHello,
    in ascending message offset. offset: of the entry in the packet."""
    R, cur, found = len(rec), 0, {}
    while R - cur >= 4:
        m = rec[cur:]
        D = len(m)
        if D >= 16 and (m[:5] == bytes(5) or m[1] >= 1):
            break
        if m[0] not in KNOWN_TYPES:
            break
        M = min(4 + _be16(m, 2), D)
        if m[0] in (1, 2) and m[0] not in found:
            found[m[0]] = hello_of(m, M, m[0], layer, offset + 5 + cur)
        cur += M
    return sorted(found.values(), key=lambda h: h.msg_offset)


@dataclass
class Message:
    index: int
    layer_offset: int
    payload_len: int
    src_port: int
    dst_port: int
    ssl_port: int
    counts: dict
    flags: int
    hellos: list


def message(index: int, pk: bytes, layers, n_layers: int, kinds: int) -> Message | None:
    """Rules 3-7 over an in-bounds packet with a whole chain; None: no followed entry."""
    cap, msg = len(pk), None
    for k in range(n_layers):
        e = layers[k]
        o, h, L = int(e["offset"]), int(e["hdr_len"]), int(e["data_len"])
        if int(e["proto"]) != P_SSL or L < 5 or h < 5 or h > L or o + L > cap:
            continue
        if msg is None:
            sp = dp = 0
            fl = abi.SSL_NO_TCP
            if k > 0 and int(layers[k - 1]["proto"]) == P_TCP and int(layers[k - 1]["offset"]) + 4 <= cap:
                t = int(layers[k - 1]["offset"])
                sp, dp, fl = _be16(pk, t), _be16(pk, t + 2), 0
            msg = Message(index, o, L, sp, dp, sp if sp in SSL_PORTS else dp, Counter(), fl, [])
        kind = pk[o]
        msg.counts[kind] += 1
        if kind == HANDSHAKE:
            msg.hellos += [x for x in handshake_hellos(pk[o + 5:o + h], k, o) if (kinds >> (x.kind - 1)) & 1]
    return msg


@dataclass
class Result:
    """What a call writes: totals always; the rest None / empty on overflow."""
    totals: list
    disposition: list | None = None
    msgs: list = field(default_factory=list)    # rows of abi.SSL_MSG_DTYPE
    hellos: list = field(default_factory=list)  # rows of abi.SSL_HELLO_DTYPE
    names: bytes = b""
    messages: list = field(default_factory=list)  # the Message objects, whatever the capacities


def model(data, offsets, caplens, data_len: int, flags, n_layers, layers, max_layers: int, kinds: int = 3,
          max_msgs: int = 0, out_msgs: int | None = None, out_hellos: int | None = None, names_cap: int | None = None,
          want_names: bool = True) -> Result:
    """The ssl contract over a batch: data (u8 array), the descriptors, the records' flags / n_layers columns and the
    FIXED layer array [n, max_layers]. out_msgs / out_hellos / names_cap None: always enough."""
    n = len(caplens)
    disp, found = [], []
    for i in range(n):
        off, cap = int(offsets[i]), int(caplens[i])
        if off + cap > data_len:
            disp.append(abi.SSL_BAD_DESC)
            continue
        if incomplete_chain(int(flags[i]), int(n_layers[i]), max_layers):
            disp.append(abi.SSL_HOST)
            continue
        m = message(i, bytes(data[off:off + cap]), layers[i], int(n_layers[i]), kinds)
        disp.append(abi.SSL_NONE if m is None else abi.SSL_MSG)
        if m is not None:
            found.append(m)
    msgs, recs, out = [], [], bytearray()
    sat = lambda v: min(v, 255)  # noqa: E731
    for j, m in enumerate(found):
        first, pos0 = len(recs), len(out)
        for h in m.hellos:
            recs.append((len(out), j, h.msg_offset & 0xFFFF, len(h.name), h.version, h.header_version, h.cipher,
                         h.n_ciphers, h.n_ext, h.kind, h.layer, h.sid, h.flags, (0, 0)))
            out += h.name
        msgs.append((first, m.index, len(out) - pos0, m.layer_offset, m.payload_len, m.src_port, m.dst_port,
                     m.ssl_port, sat(m.counts[HANDSHAKE]), sat(m.counts[CCS]), sat(m.counts[ALERT]),
                     sat(m.counts[APPDATA]), len(m.hellos), m.flags))
    totals = [0] * abi.SSL_TOTALS
    totals[abi.SSL_MSGS] = len(found)
    totals[abi.SSL_HELLOS] = len(recs)
    totals[abi.SSL_CLIENT_HELLOS] = sum(1 for r in recs if r[9] == abi.SSL_CLIENT)
    totals[abi.SSL_SERVER_HELLOS] = sum(1 for r in recs if r[9] == abi.SSL_SERVER)
    totals[abi.SSL_NAME_BYTES] = len(out)
    totals[abi.SSL_HOST_N] = disp.count(abi.SSL_HOST)
    totals[abi.SSL_BAD_DESC_N] = disp.count(abi.SSL_BAD_DESC)
    totals[abi.SSL_PAYLOAD_BYTES] = sum(m.payload_len for m in found)
    totals[abi.SSL_ALERT_PKTS] = sum(1 for m in found if m.counts[ALERT])
    totals[abi.SSL_APPDATA_PKTS] = sum(1 for m in found if m.counts[APPDATA])
    if len(found) > (max_msgs or n) or (out_msgs is not None and len(found) > out_msgs) or \
            (out_hellos is not None and len(recs) > out_hellos) or \
            (want_names and names_cap is not None and len(out) > names_cap):
        totals[abi.SSL_OVERFLOW] = 1
        return Result(totals, None, messages=found)
    return Result(totals, disp, msgs, recs, bytes(out) if want_names else b"", found)


def msgs_array(msgs: list) -> np.ndarray:
    """A model Result's messages as abi.SSL_MSG_DTYPE."""
    out = np.zeros(len(msgs), abi.SSL_MSG_DTYPE)
    for k, m in enumerate(msgs):
        out[k] = m
    return out


def hellos_array(recs: list) -> np.ndarray:
    """A model Result's hello records as abi.SSL_HELLO_DTYPE."""
    out = np.zeros(len(recs), abi.SSL_HELLO_DTYPE)
    for k, r in enumerate(recs):
        out[k] = r
    return out


# ------------------------------------------------------------------ the tables
def rows(msgs, hellos, names) -> list[tuple]:
    """One row per hello record: (source packet, kind, version, cipher, n_ciphers, n_ext, session_id_len, flags, the
    host name's bytes where the call wrote the names, else b""). msgs: abi.SSL_MSG_DTYPE; hellos: abi.SSL_HELLO_DTYPE;
    names: the call's name bytes."""
    names = bytes(names)
    out = []
    for r in hellos:
        pos = int(r["name_pos"])
        out.append((int(msgs[int(r["msg"])]["index"]), int(r["kind"]), int(r["version"]), int(r["cipher"]),
                    int(r["n_ciphers"]), int(r["n_ext"]), int(r["session_id_len"]), int(r["flags"]),
                    names[pos:pos + int(r["name_len"])]))
    return out


def _esc(b: bytes) -> str:
    return b.decode("latin-1").encode("unicode_escape").decode("ascii")


def format_row(row: tuple) -> str:
    """A row as a line of text: the host name with the bytes outside printable ASCII escaped."""
    pkt, kind, version, cipher, n_ciphers, n_ext, sid, fl, name = row
    return "\t".join([str(pkt), "server" if kind == abi.SSL_SERVER else "client", f"0x{version:04x}", f"0x{cipher:04x}",
                      str(n_ciphers), str(n_ext), str(sid), str(fl), _esc(name)])


def analyze(msgs, hellos, names, hash5) -> dict:
    """SSLAnalyzer's tables (Examples/SSLAnalyzer/SSLStatsCollector.h:271-401) from the records of a call with kinds 3
    and names written; hash5: the parse's flow key per source packet (pcppx_summary.hash5), which keys the flows as
    hash5Tuple does at :282-299. Packets, flows, total data and their per-flow averages; client and server hello
    counts; the flows with a completed handshake (the first application-data record of a flow) and with an alert; the
    ssl_port of every new flow; the version and the cipher suite id of every ServerHello; the host name of every
    ClientHello with HAS_SNI (keys with the bytes outside printable ASCII escaped).

    Cipher suites are counted by id: the reference's table of suite names is not restated here. A ServerHello whose
    id that table lacks is counted by the analyzer's version table but not by its cipher table (getCipherSuite()
    returns null there), so "ciphers" can hold ids the analyzer's report leaves out; so can a ServerHello without
    HAS_CIPHER, which is counted here under no id at all. The analyzer reads a packet only when it has a TCP layer: a
    message with SSL_NO_TCP is skipped."""
    names = bytes(names)
    out = {"packets": 0, "flows": 0, "data": 0, "client_hellos": 0, "server_hellos": 0, "handshake_complete": 0,
           "alerts": 0, "ports": Counter(), "versions": Counter(), "ciphers": Counter(), "hosts": Counter()}
    flows: dict = {}
    for m in msgs:
        if int(m["flags"]) & abi.SSL_NO_TCP:
            continue
        key = int(hash5[int(m["index"])])
        out["packets"] += 1
        out["data"] += int(m["payload_len"])
        if key not in flows:
            flows[key] = [False, False]
            out["ports"][int(m["ssl_port"])] += 1
        f = flows[key]
        if int(m["n_alert"]) and not f[0]:
            f[0] = True
            out["alerts"] += 1
        if int(m["n_appdata"]) and not f[1]:
            f[1] = True
            out["handshake_complete"] += 1
        for h in hellos[int(m["first_hello"]):int(m["first_hello"]) + int(m["n_hellos"])]:
            if int(h["kind"]) == abi.SSL_CLIENT:
                out["client_hellos"] += 1
                if int(h["flags"]) & abi.SSL_HAS_SNI:
                    pos = int(h["name_pos"])
                    out["hosts"][_esc(names[pos:pos + int(h["name_len"])])] += 1
            else:
                out["server_hellos"] += 1
                out["versions"][int(h["version"])] += 1
                if int(h["flags"]) & abi.SSL_HAS_CIPHER:
                    out["ciphers"][int(h["cipher"])] += 1
    out["flows"] = len(flows)
    out["packets_per_flow"] = out["packets"] / len(flows) if flows else 0.0
    out["data_per_flow"] = out["data"] / len(flows) if flows else 0.0
    return {k: dict(v) if isinstance(v, Counter) else v for k, v in out.items()}
