"""DNS messages in plain Python: builders, the independent model of the dns contract and the per-resource rows.

DnsLayer::parseResources links one IDnsResource per query / answer / authority / additional of a message and
IDnsResource::decodeName decodes its name (Packet++/src/DnsLayer.cpp:133-220, DnsResource.cpp:33-155); the dns mode of
Examples/PcapPlusPlus-benchmark/benchmark.cpp walks the queries and answers. pcppx_dns_device / pcppx_dns_reference
produce one record per message and per linked resource (include/pcppx.h, dns). This module holds

  name() / labels() / pointer() / question() / record() / message() / udp_packet() / tcp_packet()
             crafted names (labels, compression pointers, raw label bytes), resources, messages and packets for the
             tests and the benchmark,
  model()    the dns contract restated packet by packet over Python integers and byte strings, with decodeName as the
             recursion the reference has: it shares no code with the C++ / HIP implementation and is what the tests
             compare pcppx_dns_reference with,
  rows()     messages, resource records and names turned into one row per resource: the packet, section, name, type,
             class, TTL, data length.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from . import abi

P_DNS, P_TCP = 13, 4  # pcpp::DNS, pcpp::TCP
HEADER = 12           # sizeof(dnshdr)
MAX_RESOURCES = 300   # DnsLayer.cpp:145
TYPE_A, TYPE_NS, TYPE_CNAME, TYPE_PTR, TYPE_MX, TYPE_TXT, TYPE_AAAA, TYPE_OPT = 1, 2, 5, 12, 15, 16, 28, 41
CLASS_IN = 1
SECTION_NAMES = ("query", "answer", "authority", "additional")


# ------------------------------------------------------------------ builders
def labels(*parts: bytes) -> bytes:
    """Raw labels, each behind its length byte, without a terminator (any bytes, any length up to 255)."""
    return b"".join(bytes([len(p)]) + p for p in parts)


def pointer(to: int) -> bytes:
    """A compression pointer to byte `to` of the message (before the TCP adjustment)."""
    return bytes([0xC0 | (to >> 8) & 0x3F, to & 0xFF])


def name(text: str | bytes, to: int | None = None) -> bytes:
    """An encoded name: the dotted labels, then a zero byte or, with `to`, a pointer."""
    raw = text.encode() if isinstance(text, str) else text
    body = labels(*[p for p in raw.split(b".") if p]) if raw else b""
    return body + (b"\0" if to is None else pointer(to))


def question(qname: bytes, type_: int = TYPE_A, class_: int = CLASS_IN) -> bytes:
    return qname + struct.pack(">HH", type_, class_)


def record(rname: bytes, type_: int = TYPE_A, data: bytes = b"\x7f\0\0\1", ttl: int = 300, class_: int = CLASS_IN,
           data_len: int | None = None) -> bytes:
    """A resource record; data_len: the length field when it shall not be len(data)."""
    return rname + struct.pack(">HHIH", type_, class_, ttl, len(data) if data_len is None else data_len) + data


def message(questions=(), answers=(), authorities=(), additionals=(), id_: int = 0x1234, flags: int = 0x8180,
            counts=None, tail: bytes = b"") -> bytes:
    """A DNS message: the 12-byte header and the encoded resources back to back. counts: the four header counts when
    they shall not be the numbers of resources given."""
    c = counts if counts is not None else (len(questions), len(answers), len(authorities), len(additionals))
    return struct.pack(">HHHHHH", id_, flags, *c) + b"".join(questions) + b"".join(answers) + \
        b"".join(authorities) + b"".join(additionals) + tail


def tcp_framed(msg: bytes, length: int | None = None) -> bytes:
    """The two length bytes DNS over TCP puts in front of a message."""
    return struct.pack(">H", len(msg) if length is None else length) + msg


_MAC = bytes.fromhex("020000000001020000000002")


def _ip(proto: int, payload: bytes, k: int, from_server: bool) -> bytes:
    ca, sa = 0x0A000000 + 1 + k % 250, 0xC0A80001 + (k // 250) % 250
    src, dst = (sa, ca) if from_server else (ca, sa)
    return _MAC + b"\x08\x00" + struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(payload), k & 0xFFFF, 0x4000, 64, proto, 0,
                                            src, dst) + payload


def udp_packet(msg: bytes, k: int = 0, from_server: bool = True, port: int = 53) -> bytes:
    """Ethernet / IPv4 / UDP around a DNS message, client port 40000 + k % 1000; the message starts at byte 42."""
    cp = 40000 + k % 1000
    sport, dport = (port, cp) if from_server else (cp, port)
    return _ip(17, struct.pack(">HHHH", sport, dport, 8 + len(msg), 0) + msg, k, from_server)


def tcp_packet(payload: bytes, k: int = 0, from_server: bool = True, port: int = 53) -> bytes:
    """Ethernet / IPv4 / TCP around a payload (tcp_framed() for DNS); the payload starts at byte 54."""
    cp = 40000 + k % 1000
    sport, dport = (port, cp) if from_server else (cp, port)
    return _ip(6, struct.pack(">HHIIBBHHH", sport, dport, 1000 + k, 2000 + k, 0x50, 0x18, 512, 0, 0) + payload, k,
               from_server)


# ------------------------------------------------------------------ the contract (include/pcppx.h, dns), restated
def _be16(b: bytes, at: int) -> int:
    return (b[at] << 8) | b[at + 1]


def decode_name(d: bytes, L: int, off: int, adj: int, level: int = 1):
    """Rule 5, IDnsResource::decodeName as it recurses: (name_len, text, ok). d: the layer's bytes. A resource's own
    name is level 1 (the default of the reference's `iteration` argument, DnsResource.h:43)."""
    if off + 1 > L or level > 20:
        return 0, b"", True
    enc, text, cur = 0, bytearray(), off

    def finish():  # cleanup(): a zero label, or a pointer cut by the layer's end
        n = len(text)
        return enc + (1 if n < 256 else 0), bytes(text[:-1] if n else text), True

    def cut():     # the next label leaves the layer or passes 255 encoded bytes
        return (256, bytes(text[:-1]), True) if enc == 256 else (enc + 1, bytes(text), True)

    while d[cur] != 0:
        w = d[cur]
        if w & 0xC0 == 0xC0:
            if cur + 2 > L or enc > 255:
                return finish()
            to = (((w & 0x3F) << 8 | d[cur + 1]) + adj) & 0xFFFF
            if to < HEADER or to >= L:
                return 0, bytes(text), False       # illegal pointer: this level fails, its labels so far stay
            _, tail, _ = decode_name(d, L, to, adj, level + 1)
            tail = tail.split(b"\0")[0]            # the caller copies a C string
            text += tail[:max(0, 255 - len(text))]
            return enc + 2, bytes(text), True      # no trailing-dot removal on this path
        if cur + w + 1 > L or enc + w > 255:
            return cut()
        text += d[cur + 1:cur + 1 + w] + b"."
        cur += w + 1
        enc += w + 1
        if cur + 1 > L:
            return cut()
    return finish()


def resource_name(d: bytes, L: int, off: int, adj: int):
    """(name_len, the resource's name): empty when the decode failed or name_len is 0, else a C string's bytes."""
    name_len, text, ok = decode_name(d, L, off, adj)
    return name_len, (b"" if not ok or name_len == 0 else text.split(b"\0")[0])


def dns_layer(cap: int, layers, n_layers: int, max_layers: int):
    """Rule 2: None without an entry of proto 13; else (offset, L, adj), or False for an entry that is not followed."""
    for k in range(min(n_layers, max_layers)):
        e = layers[k]
        if int(e["proto"]) != P_DNS:
            continue
        o, h, L = int(e["offset"]), int(e["hdr_len"]), int(e["data_len"])
        adj = 2 if k >= 1 and int(layers[k - 1]["proto"]) == P_TCP else 0
        return (o, L, adj) if h <= L and o + L <= cap and L >= HEADER + adj else False
    return None


def needs_host(flags: int, n_layers: int, max_layers: int) -> bool:
    """Rule 3."""
    if flags & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW):
        return True
    if n_layers > max_layers:
        return True
    return bool(flags & abi.F_NEEDS_HOST_L7) and (bool(flags & abi.F_L7_DNS) or not flags & abi.F_L7_KNOWN)


@dataclass
class Resource:
    section: int
    offset: int
    name_len: int
    name: bytes
    type: int
    dns_class: int
    ttl: int
    data_len: int
    data_offset: int
    size: int


@dataclass
class Message:
    index: int
    layer_offset: int
    layer_len: int
    adjust: int
    id: int
    flags: int
    declared: tuple
    status: int
    resources: list  # every linked Resource, in walk order


def walk(d: bytes, L: int, adj: int):
    """Rule 4 over the layer's bytes: (declared, status, linked resources)."""
    declared = tuple(_be16(d, adj + 4 + 2 * k) for k in range(4))
    if sum(declared) > MAX_RESOURCES:
        return declared, abi.DNS_TOO_MANY, []
    left, off, out = list(declared), HEADER + adj, []
    for _ in range(sum(declared)):
        sec = next(k for k in range(4) if left[k])
        left[sec] -= 1
        name_len, text = resource_name(d, L, off, adj)
        if sec == 0:
            dl, size = 0, name_len + 4
        else:
            at = off + name_len + 8
            dl = 0 if at >= L - 1 else _be16(d, at)
            size = name_len + 10 + dl
        if off + size > L:
            return declared, abi.DNS_TRUNCATED, out
        f = off + name_len
        ttl = 0 if sec == 0 else (_be16(d, f + 4) << 16) | _be16(d, f + 6)
        out.append(Resource(sec, off, name_len, text, _be16(d, f), _be16(d, f + 2), ttl, dl,
                            0 if sec == 0 else off + name_len + 10, size))
        off += size
    return declared, abi.DNS_COMPLETE, out


@dataclass
class Result:
    """What a call writes: totals always; the rest None / empty on overflow."""
    totals: list
    disposition: list | None = None
    msgs: list = field(default_factory=list)   # rows of abi.DNS_MSG_DTYPE
    rrs: list = field(default_factory=list)    # rows of abi.DNS_RR_DTYPE
    names: bytes = b""
    messages: list = field(default_factory=list)  # the Message objects, whatever the capacities


def model(data, offsets, caplens, data_len: int, flags, n_layers, layers, max_layers: int, sections: int = 15,
          max_msgs: int = 0, out_msgs: int | None = None, out_rrs: int | None = None, names_cap: int | None = None,
          want_names: bool = True) -> Result:
    """The dns contract over a batch: data (u8 array), the descriptors, the records' flags / n_layers columns and the
    FIXED layer array [n, max_layers]. out_msgs / out_rrs / names_cap None: always enough."""
    n = len(caplens)
    disp, found = [], []
    for i in range(n):
        off, cap = int(offsets[i]), int(caplens[i])
        if off + cap > data_len:
            disp.append(abi.DNS_BAD_DESC)
            continue
        lay = dns_layer(cap, layers[i], int(n_layers[i]), max_layers)
        if lay is None:
            disp.append(abi.DNS_HOST if needs_host(int(flags[i]), int(n_layers[i]), max_layers) else abi.DNS_NONE)
            continue
        if lay is False:
            disp.append(abi.DNS_NONE)
            continue
        o, L, adj = lay
        d = bytes(data[off + o:off + o + L])
        declared, status, res = walk(d, L, adj)
        found.append(Message(i, o, L, adj, _be16(d, adj), _be16(d, adj + 2), declared, status, res))
        disp.append(abi.DNS_MSG)
    want = lambda r: (sections >> r.section) & 1  # noqa: E731
    n_rrs = sum(1 for m in found for r in m.resources if want(r))
    name_bytes = sum(len(r.name) for m in found for r in m.resources if want(r))
    totals = [0] * abi.DNS_TOTALS
    totals[abi.DNS_MSGS] = len(found)
    totals[abi.DNS_RRS] = n_rrs
    totals[abi.DNS_NAME_BYTES] = name_bytes
    totals[abi.DNS_HOST_N] = disp.count(abi.DNS_HOST)
    totals[abi.DNS_BAD_DESC_N] = disp.count(abi.DNS_BAD_DESC)
    totals[abi.DNS_QA_LINKED] = sum(1 for m in found for r in m.resources if r.section < 2)
    if len(found) > (max_msgs or n) or (out_msgs is not None and len(found) > out_msgs) or \
            (out_rrs is not None and n_rrs > out_rrs) or \
            (want_names and names_cap is not None and name_bytes > names_cap):
        totals[abi.DNS_OVERFLOW] = 1
        return Result(totals, None, messages=found)
    msgs, rrs, names = [], [], bytearray()
    for j, m in enumerate(found):
        linked = [sum(1 for r in m.resources if r.section == s) for s in range(4)]
        emitted = [r for r in m.resources if want(r)]
        msgs.append((len(rrs), m.index, m.layer_offset, m.layer_len, m.id, m.flags, m.declared, linked, len(emitted),
                     m.adjust, m.status))
        for r in emitted:
            rrs.append((len(names), j, r.ttl, r.offset, r.name_len, len(r.name), r.type, r.dns_class, r.data_len,
                        r.data_offset, r.section, 0))
            names += r.name
    return Result(totals, disp, msgs, rrs, bytes(names) if want_names else b"", found)


def msgs_array(msgs: list) -> np.ndarray:
    """A model Result's messages as abi.DNS_MSG_DTYPE."""
    out = np.zeros(len(msgs), abi.DNS_MSG_DTYPE)
    for k, m in enumerate(msgs):
        out[k] = m
    return out


def rrs_array(rrs: list) -> np.ndarray:
    """A model Result's resource records as abi.DNS_RR_DTYPE."""
    out = np.zeros(len(rrs), abi.DNS_RR_DTYPE)
    for k, r in enumerate(rrs):
        out[k] = r
    return out


# ------------------------------------------------------------------ the per-resource table
def rows(msgs, rrs, names) -> list[tuple]:
    """One row per resource record: (source packet, section, name bytes, type, class, TTL, data length). msgs:
    abi.DNS_MSG_DTYPE; rrs: abi.DNS_RR_DTYPE; names: the call's name bytes."""
    names = bytes(names)
    out = []
    for r in rrs:
        pos = int(r["name_pos"])
        out.append((int(msgs[int(r["msg"])]["index"]), int(r["section"]), names[pos:pos + int(r["text_len"])],
                    int(r["type"]), int(r["dns_class"]), int(r["ttl"]), int(r["data_len"])))
    return out


def format_row(row: tuple) -> str:
    """A row as a line of text: the name with the bytes outside printable ASCII escaped."""
    pkt, sec, nm, type_, class_, ttl, dl = row
    return "\t".join([str(pkt), SECTION_NAMES[sec], nm.decode("latin-1").encode("unicode_escape").decode("ascii"),
                      str(type_), str(class_), str(ttl), str(dl)])
