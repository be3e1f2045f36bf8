"""TLS fingerprints (JA3 / JA3S) in plain Python: builders, the independent model and the example's output.

Examples/TLSFingerprinting writes one row per ClientHello / ServerHello packet: the MD5 of the fingerprint text, the
text, the kind, and the packet's addresses and ports (main.cpp:202-211), and prints the most common fingerprints
(main.cpp:246-272). pcppx_tlsfp_device / pcppx_tlsfp_reference produce the records of those rows (include/pcppx.h,
tlsfp). This module holds

  client_hello() / server_hello() / record() / tcp_packet()   crafted messages, TLS records and packets for the tests
                                                               and the benchmark,
  model()    the tlsfp contract restated packet by packet over Python integers and byte strings with hashlib.md5: it
             shares no code with the C++ / HIP implementation and is what the tests compare pcppx_tlsfp_reference with,
  rows()     records, 5-tuple extracts and text turned into the seven columns of the example's output file,
  top()      the example's per-fingerprint counts, most common first.
"""
from __future__ import annotations

import hashlib
import ipaddress
import struct
from dataclasses import dataclass, field

import numpy as np

from . import abi

P_SSL = 18  # pcpp::SSL
HANDSHAKE, CHANGE_CIPHER_SPEC, APPLICATION_DATA = 22, 20, 23
EXT_GROUPS, EXT_FORMATS, EXT_VERSIONS = 10, 11, 43
HEADER = ("TLS Fingerprint (MD5)", "TLS Fingerprint", "TLS Fingerprint type", "IP Source", "TCP Source Port",
          "IP Dest", "TCP Dest Port")
KIND_NAMES = {abi.TLSFP_CLIENT: "ClientHello", abi.TLSFP_SERVER: "ServerHello"}
GREASE = frozenset(0x0A0A + 0x1010 * k for k in range(16))  # 0x0a0a, 0x1a1a, ... 0xfafa (SSLHandshake.cpp:1040-1053)


# ------------------------------------------------------------------ builders
def ext(type_: int, data: bytes = b"", length: int | None = None) -> bytes:
    """One extension; length: the length field when it shall not be len(data)."""
    return struct.pack(">HH", type_, len(data) if length is None else length) + data


def groups_ext(groups, list_len: int | None = None) -> bytes:
    body = b"".join(struct.pack(">H", g) for g in groups)
    return ext(EXT_GROUPS, struct.pack(">H", len(body) if list_len is None else list_len) + body)


def formats_ext(formats, list_len: int | None = None) -> bytes:
    body = bytes(formats)
    return ext(EXT_FORMATS, bytes([len(body) if list_len is None else list_len]) + body)


def _message(type_: int, body: bytes, length: int | None) -> bytes:
    ln = len(body) if length is None else length
    return bytes([type_]) + ln.to_bytes(3, "big") + body


def client_hello(ciphers=(0x1301, 0xC02F), extensions: bytes = b"", version: int = 0x0303, sid: bytes = b"",
                 compression: bytes = b"\0", length: int | None = None, cipher_bytes: int | None = None,
                 ext_len: int | None = None, sid_len: int | None = None, with_extensions: bool = True) -> bytes:
    """A ClientHello handshake message. length / cipher_bytes / ext_len / sid_len: the length fields when they shall
    not be what the content has."""
    cs = b"".join(struct.pack(">H", c) for c in ciphers)
    body = struct.pack(">H", version) + bytes(range(32)) + bytes([len(sid) if sid_len is None else sid_len]) + sid
    body += struct.pack(">H", len(cs) if cipher_bytes is None else cipher_bytes) + cs
    body += bytes([len(compression)]) + compression
    if with_extensions:
        body += struct.pack(">H", len(extensions) if ext_len is None else ext_len) + extensions
    return _message(1, body, length)


def server_hello(cipher: int = 0x1301, extensions: bytes = b"", version: int = 0x0303, sid: bytes = b"",
                 length: int | None = None, ext_len: int | None = None, with_extensions: bool = True) -> bytes:
    body = struct.pack(">H", version) + bytes(range(32)) + bytes([len(sid)]) + sid + struct.pack(">HB", cipher, 0)
    if with_extensions:
        body += struct.pack(">H", len(extensions) if ext_len is None else ext_len) + extensions
    return _message(2, body, length)


def other_message(type_: int = 11, size: int = 12) -> bytes:
    """A handshake message of another type with `size` body bytes (none of them zero)."""
    return _message(type_, bytes(1 + k % 250 for k in range(size)), None)


def record(payload: bytes, type_: int = HANDSHAKE, version: int = 0x0303, length: int | None = None) -> bytes:
    """A TLS record; length: the length field when it shall not be len(payload)."""
    return struct.pack(">BHH", type_, version, len(payload) if length is None else length) + payload


def tcp_packet(payload: bytes, k: int = 0, from_server: bool = False, v6: bool = False) -> bytes:
    """Ethernet / IP / TCP around a TLS payload, client port 50000 + k % 1000 and server port 443."""
    cp, sp = 50000 + k % 1000, 443
    sport, dport = (sp, cp) if from_server else (cp, sp)
    tcp = struct.pack(">HHIIBBHHH", sport, dport, 1000 + k, 2000 + k, 0x50, 0x18, 512, 0, 0) + payload
    ca, sa = 0x0A000000 + 1 + k % 250, 0xC0A80001 + (k // 250) % 250
    mac = bytes.fromhex("020000000001020000000002")
    if v6:
        a = lambda x: bytes.fromhex("20010db8") + bytes(8) + struct.pack(">I", x)  # noqa: E731
        src, dst = (a(sa), a(ca)) if from_server else (a(ca), a(sa))
        return mac + b"\x86\xdd" + struct.pack(">IHBB", 0x60000000, len(tcp), 6, 64) + src + dst + tcp
    src, dst = (sa, ca) if from_server else (ca, sa)
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(tcp), k & 0xFFFF, 0x4000, 64, 6, 0, src, dst)
    return mac + b"\x08\x00" + ip + tcp


# ------------------------------------------------------------------ the contract (include/pcppx.h, tlsfp), restated
def _be16(b: bytes, at: int) -> int:
    return (b[at] << 8) | b[at + 1]


def handshake_layer(pkt: bytes, layers, n_layers: int, max_layers: int):
    """Rule 2: (offset, R) of the first recorded SSL layer that lies inside the packet and holds a handshake record."""
    for k in range(min(n_layers, max_layers)):
        L = layers[k]
        o, h, d = int(L["offset"]), int(L["hdr_len"]), int(L["data_len"])
        if int(L["proto"]) == P_SSL and d >= 5 and 5 <= h <= d and o + d <= len(pkt) and pkt[o] == HANDSHAKE:
            return o, h - 5
    return None


def needs_host(flags: int, n_layers: int, max_layers: int) -> bool:
    """Rule 3."""
    if flags & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW):
        return True
    if n_layers > max_layers:
        return True
    return bool(flags & abi.F_NEEDS_HOST_L7) and (bool(flags & abi.F_L7_SSL) or not flags & abi.F_L7_KNOWN)


def messages(pkt: bytes, offset: int, R: int):
    """Rule 4: [(type, start, D, M)] of the known messages of the record, in order."""
    out, cur = [], 0
    while R - cur >= 4:
        D, at = R - cur, offset + 5 + cur
        if D >= 16 and (pkt[at:at + 5] == bytes(5) or pkt[at + 1] >= 1):
            break
        M = min(4 + _be16(pkt, at + 2), D)
        out.append((pkt[at], at, D, M))
        cur += M
    return out


def extension_list(m: bytes, D: int, M: int, E: int):
    """Rule 5: [(type, data)] of the extension list whose length field is at E. m: the message's D readable bytes."""
    if E + 2 > D:
        return []
    it = E + 2
    end = min(it + _be16(m, E), M)
    out = []
    while end - it >= 4:
        t, ln = _be16(m, it), _be16(m, it + 2)
        if end - it < 4 + ln:
            break
        out.append((t, m[it + 4:it + 4 + ln]))
        it += 4 + ln
    return out


def _session_id(m: bytes, D: int) -> int:
    return 0 if D <= 39 else min(m[38], D - 39)


def _join(values) -> str:
    return "-".join(str(v) for v in values)


def client_text(m: bytes, D: int, M: int) -> str:
    """Rule 6. m: the bytes from the message's first byte to the record's end (D of them)."""
    version = 0 if D < 6 else _be16(m, 4)
    cs = 39 + _session_id(m, D)
    count = 0 if cs + 2 > D else _be16(m, cs) // 2
    ciphers = [_be16(m, cs + 2 + 2 * i) for i in range(count) if cs + 2 + 2 * (i + 1) <= D]
    exts = extension_list(m, D, M, cs + 2 + 2 * count + 2)
    groups, formats = [], []
    for t, data in exts:
        if t == EXT_GROUPS:
            if len(data) >= 2 and _be16(data, 0) == len(data) - 2 and _be16(data, 0) % 2 == 0:
                groups = [_be16(data, 2 + 2 * j) for j in range(_be16(data, 0) // 2)]
            break
    for t, data in exts:
        if t == EXT_FORMATS:
            if len(data) >= 1 and len(data) == data[0] + 1:
                formats = list(data[1:])
            break
    keep = lambda vs: [v for v in vs if v not in GREASE]  # noqa: E731
    return ",".join([str(version), _join(keep(ciphers)), _join(keep([t for t, _ in exts])), _join(keep(groups)),
                     _join(formats)])


def server_text(m: bytes, D: int, M: int) -> str:
    """Rule 7."""
    version = 0 if D < 6 else _be16(m, 4)
    at = 39 + _session_id(m, D)
    cipher = 0 if at + 2 > D else _be16(m, at)
    exts = extension_list(m, D, M, at + 3)
    for t, data in exts:
        if t == EXT_VERSIONS:
            if len(data) == 2:
                version = _be16(data, 0)
            elif len(data) == 3 and data[0] == 2:
                version = _be16(data, 1)
            break
    return ",".join([str(version), str(cipher), _join(t for t, _ in exts)])


@dataclass
class Result:
    """What a call writes: totals always; the rest None on overflow."""
    totals: list
    disposition: list | None = None
    recs: list = field(default_factory=list)  # (md5 bytes, text_pos, text_len, index, msg_offset & 0xFFFF, kind)
    text: bytes = b""


def classify(pkt: bytes, flags: int, n_layers: int, layers, max_layers: int, client: bool, server: bool):
    """Rules 2-4 for an in-bounds packet: (disposition, text or None, message offset)."""
    found = handshake_layer(pkt, layers, n_layers, max_layers)
    if found is None:
        return (abi.TLSFP_HOST if needs_host(flags, n_layers, max_layers) else abi.TLSFP_NONE), None, 0
    offset, R = found
    msgs = messages(pkt, offset, R)
    for want, kind, text_of in ((client, abi.TLSFP_CLIENT, client_text), (server, abi.TLSFP_SERVER, server_text)):
        if not want:
            continue
        for type_, at, D, M in msgs:
            if type_ == kind:  # the message types are 1 and 2, as the kinds
                return kind, text_of(pkt[at:at + D], D, M), at
    return abi.TLSFP_NONE, None, 0


def model(data, offsets, caplens, data_len: int, flags, n_layers, layers, max_layers: int, client: bool = True,
          server: bool = True, max_hellos: int = 0, max_recs: int | None = None, text_cap: int | None = None,
          want_text: bool = True) -> Result:
    """The tlsfp contract over a batch: data (u8 array), the descriptors, the records' flags / n_layers columns and the
    FIXED layer array [n, max_layers]. max_recs / text_cap None: always enough."""
    n = len(caplens)
    disp, found = [], []
    for i in range(n):
        off, cap = int(offsets[i]), int(caplens[i])
        if off + cap > data_len:
            disp.append(abi.TLSFP_BAD_DESC)
            continue
        pkt = bytes(data[off:off + cap])
        d, text, at = classify(pkt, int(flags[i]), int(n_layers[i]), layers[i], max_layers, client, server)
        disp.append(d)
        if text is not None:
            found.append((i, d, at, text.encode()))
    totals = [0] * abi.TLSFP_TOTALS
    totals[abi.TLSFP_HOST_N] = disp.count(abi.TLSFP_HOST)
    totals[abi.TLSFP_BAD_DESC_N] = disp.count(abi.TLSFP_BAD_DESC)
    totals[abi.TLSFP_CANDIDATES] = len(found)
    if len(found) > (max_hellos or n):
        totals[abi.TLSFP_OVERFLOW] = 1
        return Result(totals, None)
    totals[abi.TLSFP_CLIENT_N] = disp.count(abi.TLSFP_CLIENT)
    totals[abi.TLSFP_SERVER_N] = disp.count(abi.TLSFP_SERVER)
    totals[abi.TLSFP_TEXT_BYTES] = sum(len(f[3]) for f in found)
    if (max_recs is not None and len(found) > max_recs) or \
            (want_text and text_cap is not None and totals[abi.TLSFP_TEXT_BYTES] > text_cap):
        totals[abi.TLSFP_OVERFLOW] = 1
        return Result(totals, None)
    recs, pos = [], 0
    for i, kind, at, text in found:
        recs.append((hashlib.md5(text).digest(), pos, len(text), i, at & 0xFFFF, kind))
        pos += len(text)
    return Result(totals, disp, recs, b"".join(f[3] for f in found) if want_text else b"")


# ------------------------------------------------------------------ the example's output
def _address(raw, version: int) -> str:
    if version == 4:
        return str(ipaddress.IPv4Address(bytes(raw[:4])))
    if version == 6:
        return str(ipaddress.IPv6Address(bytes(raw)))
    return "0.0.0.0"  # a default-constructed pcpp::IPAddress


def rows(recs, tuples, text) -> list[tuple]:
    """The seven columns of the example's output file (main.cpp:202-211), one tuple of strings per record. recs:
    abi.TLSFP_REC_DTYPE; tuples: the parse's abi.TUPLE_DTYPE extracts of the whole batch (recs["index"] indexes them;
    ports are those of the TCP layer, 0 where the port layer is not TCP); text: the call's text bytes."""
    text = bytes(text)
    out = []
    for r in recs:
        t = tuples[int(r["index"])]
        tcp = int(t["l4_proto"]) == 4
        pos = int(r["text_pos"])
        out.append((bytes(r["md5"]).hex(), text[pos:pos + int(r["text_len"])].decode("ascii"),
                    KIND_NAMES[int(r["kind"])], _address(t["src_ip"], int(t["ip_version"])),
                    str(int(t["src_port"]) if tcp else 0), _address(t["dst_ip"], int(t["ip_version"])),
                    str(int(t["dst_port"]) if tcp else 0)))
    return out


def write_rows(path, table: list[tuple], separator: str = "\t") -> None:
    """The example's output file: the column headers (main.cpp:216-221), then one line per row."""
    with open(path, "w") as f:
        for row in [HEADER] + list(table):
            f.write(separator.join(row) + "\n")


def top(recs, kind: int, count: int | None = 10) -> list[tuple[str, int]]:
    """The example's table of the most common fingerprints of one kind (main.cpp:246-272): (md5 hex, packets), by
    count and then by the hex string, both descending (stringCountComparer, main.cpp:63-70); count None: all."""
    seen: dict[str, int] = {}
    for r in recs:
        if int(r["kind"]) == kind:
            h = bytes(r["md5"]).hex()
            seen[h] = seen.get(h, 0) + 1
    ranked = sorted(seen.items(), key=lambda kv: (kv[1], kv[0]), reverse=True)
    return ranked if count is None else ranked[:count]


def records_array(recs: list) -> np.ndarray:
    """A model Result's records as abi.TLSFP_REC_DTYPE."""
    out = np.zeros(len(recs), abi.TLSFP_REC_DTYPE)
    for k, (md5, pos, ln, idx, at, kind) in enumerate(recs):
        out[k] = (np.frombuffer(md5, np.uint8), pos, ln, idx, at, kind, np.zeros(5, np.uint8))
    return out
