"""DHCP and DHCPv6 messages in plain Python: builders, the independent model of the dhcp contract, the per-option rows,
the lease table and the client fingerprints.

The reference builds a DhcpLayer behind UDP from the port pairs 68->67, 67->68 and 67->67, and a DhcpV6Layer from a port
546 / 547 further down the same dispatch (Packet++/src/UdpLayer.cpp:103-141); both read their options with the same
TLVRecordReader (Packet++/header/TLVData.h). pcppx_dhcp_device / pcppx_dhcp_reference produce one record per message
and per option the caller asks for (include/pcppx.h, dhcp). This module holds

  opt4() / bootp() / opt6() / message6() / packet()
                  crafted messages and packets for the tests and the benchmark,
  model()         the dhcp contract restated packet by packet over Python byte strings with slices and struct: it
                  shares no code with the C++ / HIP implementation and is what the tests compare pcppx_dhcp_reference
                  with,
  rows()          messages, option records and values turned into one row per message and option,
  leases()        the MAC <-> address <-> lease table from the DHCPv4 ACKs of a call,
  fingerprints()  the option 55 list and the option 60 text of every DHCPv4 DISCOVER / REQUEST.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .sip import packet as udp_packet

P_UDP, P_TRAILER = 5, 30  # pcpp::UDP, pcpp::PacketTrailer
MAGIC = bytes((0x63, 0x82, 0x53, 0x63))
DISCOVER, OFFER, REQUEST, DECLINE, ACK, NAK, RELEASE, INFORM = range(1, 9)
HOST_OTHER_PORTS = frozenset((1812, 1813, 3799, 2152, 2123))  # rule 6: RADIUS and GTP come before DHCPv6


# ------------------------------------------------------------------ builders
def opt4(code: int, value: bytes = b"", length: int | None = None) -> bytes:
    """A DHCPv4 option; PAD (0) and END (255) are the single byte. length: the length byte, when it shall lie."""
    if code in (0, 255):
        return bytes([code])
    return bytes([code, len(value) if length is None else length]) + value


def bootp(op: int = 1, xid: int = 0x12345678, mac: bytes = bytes.fromhex("020000000001"), options: bytes = b"",
          ciaddr: str = "0.0.0.0", yiaddr: str = "0.0.0.0", siaddr: str = "0.0.0.0", giaddr: str = "0.0.0.0",
          secs: int = 0, flags: int = 0, htype: int = 1, hlen: int = 6, hops: int = 0, magic: bytes = MAGIC) -> bytes:
    """The 240-byte BOOTP header (the magic number included) and the options behind it."""
    ip = lambda a: bytes(int(x) for x in a.split("."))  # noqa: E731
    return struct.pack(">BBBBIHH", op, htype, hlen, hops, xid, secs, flags) + ip(ciaddr) + ip(yiaddr) + ip(siaddr) + \
        ip(giaddr) + mac.ljust(16, b"\0")[:16] + bytes(64) + bytes(128) + magic + options


def message4(msg_type: int, options: list | bytes = (), end: bool = True, **kw) -> bytes:
    """A DHCPv4 message: option 53 first, then options ((code, value) pairs or raw bytes), then END."""
    raw = options if isinstance(options, bytes) else b"".join(o if isinstance(o, bytes) else opt4(*o) for o in options)
    kw.setdefault("op", 2 if msg_type in (OFFER, ACK, NAK) else 1)
    return bootp(options=opt4(53, bytes([msg_type])) + raw + (opt4(255) if end else b""), **kw)


def opt6(code: int, value: bytes = b"", length: int | None = None) -> bytes:
    return struct.pack(">HH", code, len(value) if length is None else length) + value


def message6(msg_type: int = 1, xid: int = 0xABCDEF, options: list | bytes = ()) -> bytes:
    raw = options if isinstance(options, bytes) else b"".join(o if isinstance(o, bytes) else opt6(*o) for o in options)
    return bytes([msg_type]) + xid.to_bytes(3, "big") + raw


def packet(payload: bytes, k: int = 0, sport: int = 68, dport: int = 67, **kw) -> bytes:
    """Ethernet / IPv4 / UDP around a payload (pcapplusplus_amd.sip.packet): the payload starts at byte 42."""
    return udp_packet(payload, k, sport=sport, dport=dport, **kw)


# ------------------------------------------------------------------ the contract (include/pcppx.h, dhcp), restated
HOST = "host"


def family_of(sport: int, dport: int, L: int):
    """Rules 5-6 over the ports and the payload length: None, HOST, 4 or 6."""
    if (sport, dport) in ((68, 67), (67, 68), (67, 67)):
        return 4 if L >= 240 else None
    six = {546, 547}
    if sport not in six and dport not in six:
        return None
    if dport == 4789 or {sport, dport} & {5060, 5061}:
        return None
    if {sport, dport} & HOST_OTHER_PORTS:
        return HOST
    return 6 if L >= 4 else None


def find_layer(pkt: bytes, layers, n_layers: int, max_layers: int, flags: int):
    """Rules 2-6: None, HOST or (offset, L, family)."""
    if flags & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW) or \
            n_layers > max_layers or (flags & abi.F_NEEDS_HOST_L7 and not flags & abi.F_L7_KNOWN):
        return HOST
    if not flags & abi.F_NEEDS_HOST_L7 or flags & (abi.F_L7_HTTP | abi.F_L7_SSL | abi.F_L7_DNS):
        return None
    protos = [int(layers[k]["proto"]) for k in range(n_layers)]
    if P_UDP not in protos:
        return None
    k = len(protos) - 1 - protos[::-1].index(P_UDP)
    if protos[k + 1:] not in ([], [P_TRAILER]):
        return None
    o, h, dl = (int(layers[k][f]) for f in ("offset", "hdr_len", "data_len"))
    if h != 8 or dl <= 8 or o + dl > len(pkt):
        return None
    sport, dport = struct.unpack(">HH", pkt[o:o + 4])
    fam = family_of(sport, dport, dl - 8)
    if fam is None or fam == HOST:
        return fam
    return o + 8, dl - 8, fam


def options4(d: bytes) -> list[tuple]:
    """Rule 8: (code, len, offset) of every counted option."""
    out, rest, at = [], d[240:], 240
    while rest:
        t = rest[0]
        if t in (0, 255):
            size, ln = 1, 0
        elif len(rest) < 2:
            break
        else:
            ln = rest[1]
            size = 2 + ln
        if size > len(rest):
            break
        out.append((t, ln, at))
        rest, at = rest[size:], at + size
    return out


def options6(d: bytes) -> list[tuple]:
    """Rule 9."""
    out, at = [], 4
    while len(d) - at >= 4:
        code, ln = struct.unpack_from(">HH", d, at)
        if at + 4 + ln > len(d):
            break
        out.append((code, ln, at))
        at += 4 + ln
    return out


@dataclass
class Message:
    index: int
    layer_offset: int
    family: int
    d: bytes
    options: list  # (code, len, offset, value offset) of every counted option

    def first(self, code: int):
        for o in self.options:
            if o[0] == code:
                return o
        return None

    def value(self, o) -> bytes:
        return self.d[o[3]:o[3] + o[1]]


def message(index: int, layer_offset: int, family: int, d: bytes) -> Message:
    head = (lambda t: 1 if t in (0, 255) else 2) if family == 4 else (lambda t: 4)
    return Message(index, layer_offset, family, d,
                   [(c, ln, at, at + head(c)) for c, ln, at in (options4(d) if family == 4 else options6(d))])


def header_row(m: Message) -> dict:
    """Rule 11 and the header fields: what a message record holds besides its positions and counts."""
    d, z4 = m.d, [0, 0, 0, 0]
    r = dict(xid=0, lease_time=0, secs=0, bootp_flags=0, family=m.family, msg_type=0, flags=0, op=0, htype=0, hlen=0,
             hops=0, ciaddr=z4, yiaddr=z4, siaddr=z4, giaddr=z4, server_id=z4, client_mac=[0] * 6)
    if m.family == 6:
        r["msg_type"] = d[0] if d[0] <= 13 else 0
        r["xid"] = int.from_bytes(d[1:4], "big")
        return r
    op, htype, hlen, hops, xid, secs, fl = struct.unpack_from(">BBBBIHH", d, 0)
    r.update(op=op, htype=htype, hlen=hlen, hops=hops, xid=xid, secs=secs, bootp_flags=fl, ciaddr=list(d[12:16]),
             yiaddr=list(d[16:20]), siaddr=list(d[20:24]), giaddr=list(d[24:28]))
    flags = abi.DHCP_REPLY if op == 2 else 0
    if htype == 1 and hlen == 6:
        flags |= abi.DHCP_HAS_MAC
        r["client_mac"] = list(d[28:34])
    if d[236:240] == MAGIC:
        flags |= abi.DHCP_MAGIC_OK
    o = m.first(53)
    if o is not None:
        flags |= abi.DHCP_HAS_MSG_TYPE
        r["msg_type"] = m.value(o)[0] if o[1] >= 1 else 0
    o = m.first(51)
    if o is not None and o[1] >= 4:
        flags |= abi.DHCP_HAS_LEASE_TIME
        r["lease_time"] = int.from_bytes(m.value(o)[:4], "big")
    o = m.first(54)
    if o is not None and o[1] >= 4:
        flags |= abi.DHCP_HAS_SERVER_ID
        r["server_id"] = list(m.value(o)[:4])
    r["flags"] = flags
    return r


@dataclass
class Result:
    """What a call writes: totals always; the rest None / empty on overflow."""
    totals: list
    disposition: list | None = None
    msgs: list = field(default_factory=list)     # rows of abi.DHCP_MSG_DTYPE
    options: list = field(default_factory=list)  # rows of abi.DHCP_OPTION_DTYPE
    values: bytes = b""
    messages: list = field(default_factory=list)  # the Message objects, whatever the capacities


MSG_FIELDS = abi.DHCP_MSG_DTYPE.names


def model(data, offsets, caplens, data_len: int, flags, n_layers, layers, max_layers: int,
          codes4=abi.DHCP_ASSET_CODES4, codes6=abi.DHCP_ASSET_CODES6, options: int = abi.DHCP_OPTIONS_WANTED,
          values: int = 1, families: int = 3, max_msgs: int = 0, out_msgs: int | None = None,
          out_options: int | None = None, values_cap: int | None = None, want_values: bool = True) -> Result:
    """The dhcp contract over a batch: data (u8 array), the descriptors, the records' flags / n_layers columns and the
    FIXED layer array [n, max_layers]; codes4 / codes6: the spec's wanted codes. out_* / values_cap None: always
    enough."""
    n = len(caplens)
    want = {4: frozenset(codes4), 6: frozenset(codes6)}
    disp, found = [], []
    for i in range(n):
        off, cap = int(offsets[i]), int(caplens[i])
        if off + cap > data_len:
            disp.append(abi.DHCP_BAD_DESC)
            continue
        pkt = bytes(data[off:off + cap])
        lay = find_layer(pkt, layers[i], int(n_layers[i]), max_layers, int(flags[i]))
        if lay == HOST:
            disp.append(abi.DHCP_HOST)
            continue
        if lay is None or not families & (abi.DHCP_V4 if lay[2] == 4 else abi.DHCP_V6):
            disp.append(abi.DHCP_NONE)
            continue
        found.append(message(i, lay[0], lay[2], pkt[lay[0]:lay[0] + lay[1]]))
        disp.append(abi.DHCP_MSG)
    msgs, recs, out = [], [], bytearray()
    for j, m in enumerate(found):
        first, pos0 = len(recs), len(out)
        for ordinal, o in enumerate(m.options):
            if options == abi.DHCP_OPTIONS_NONE or (options == abi.DHCP_OPTIONS_WANTED and o[0] not in want[m.family]):
                continue
            recs.append((j, o[0], o[1], o[2], ordinal, len(out) - pos0, 0))
            if values:
                out += m.value(o)
        h = header_row(m)
        h.update(first_option=first, value_pos=pos0, index=m.index, layer_offset=m.layer_offset, layer_len=len(m.d),
                 n_options=len(m.options), n_rec=len(recs) - first, value_len=len(out) - pos0,
                 options_len=sum(o[3] - o[2] + o[1] for o in m.options), reserved0=0, reserved=[0, 0])
        msgs.append(tuple(h[f] for f in MSG_FIELDS))
    totals = [0] * abi.DHCP_TOTALS
    totals[abi.DHCP_MSGS] = len(found)
    totals[abi.DHCP_V4_N] = sum(1 for m in found if m.family == 4)
    totals[abi.DHCP_V6_N] = sum(1 for m in found if m.family == 6)
    totals[abi.DHCP_OPTIONS] = len(recs)
    totals[abi.DHCP_VALUE_BYTES] = len(out)
    totals[abi.DHCP_HOST_N] = disp.count(abi.DHCP_HOST)
    totals[abi.DHCP_BAD_DESC_N] = disp.count(abi.DHCP_BAD_DESC)
    totals[abi.DHCP_OPTIONS_LINKED] = sum(len(m.options) for m in found)
    totals[abi.DHCP_REPLIES] = sum(1 for m in found if m.family == 4 and m.d[0] == 2)
    if len(found) > (max_msgs or n) or (out_msgs is not None and len(found) > out_msgs) or \
            (out_options is not None and len(recs) > out_options) or \
            (want_values and values_cap is not None and len(out) > values_cap):
        totals[abi.DHCP_OVERFLOW] = 1
        return Result(totals, None, messages=found)
    return Result(totals, disp, msgs, recs, bytes(out) if want_values else b"", found)


def _array(rows_: list, dtype) -> np.ndarray:
    out = np.zeros(len(rows_), dtype)
    for k, r in enumerate(rows_):
        out[k] = r
    return out


def msgs_array(msgs: list) -> np.ndarray:
    """A model Result's messages as abi.DHCP_MSG_DTYPE."""
    return _array(msgs, abi.DHCP_MSG_DTYPE)


def options_array(recs: list) -> np.ndarray:
    return _array(recs, abi.DHCP_OPTION_DTYPE)


# ------------------------------------------------------------------ the tables
def _value(m, o, values: bytes) -> bytes:
    at = int(m["value_pos"]) + int(o["value_rel"])
    return values[at:at + int(o["len"])]


def _ip(b) -> str:
    return ".".join(str(int(x)) for x in b)


def _mac(b) -> str:
    return ":".join("%02x" % int(x) for x in b)


def rows(msgs, options, values, with_values: bool = True) -> list[tuple]:
    """One row per message -- (source packet, family, msg_type, None, n_options, b"") -- followed by one per option
    record of it: (source packet, family, msg_type, code, len, the value's bytes where the call copied them, else
    b""). msgs: abi.DHCP_MSG_DTYPE; options: abi.DHCP_OPTION_DTYPE."""
    values = bytes(values)
    out = []
    for m in msgs:
        key = (int(m["index"]), int(m["family"]), int(m["msg_type"]))
        out.append(key + (None, int(m["n_options"]), b""))
        first = int(m["first_option"])
        for o in options[first:first + int(m["n_rec"])]:
            v = _value(m, o, values) if with_values and int(m["value_len"]) else b""
            out.append(key + (int(o["code"]), int(o["len"]), v))
    return out


def format_row(r: tuple) -> str:
    head = f"{r[0]} v{r[1]} type={r[2]}"
    return f"{head} options={r[4]}" if r[3] is None else f"{head} opt={r[3]} len={r[4]} {r[5].hex()}"


def _by_code(m, options, values: bytes) -> dict:
    """The first value of each code among a message's emitted options."""
    first, out = int(m["first_option"]), {}
    for o in options[first:first + int(m["n_rec"])]:
        out.setdefault(int(o["code"]), _value(m, o, values))
    return out


def leases(msgs, options, values) -> list[dict]:
    """The lease table from the records of a call whose spec wanted option 12 with values: one row per DHCPv4 ACK
    (msg_type 5), in source order: the source packet, client_mac, yiaddr, lease_time (None without option 51), server_id
    (None without option 54) and host_name: option 12 of the same client's latest DISCOVER / REQUEST before the ACK in
    the batch, escaped; None when there is none."""
    values = bytes(values)
    names: dict = {}
    out = []
    for m in msgs:
        if int(m["family"]) != 4:
            continue
        mac, t = bytes(m["client_mac"]), int(m["msg_type"])
        if t in (DISCOVER, REQUEST):
            name = _by_code(m, options, values).get(12)
            if name is not None:
                names[mac] = name.decode("latin-1").encode("unicode_escape").decode("ascii")
        elif t == ACK:
            fl = int(m["flags"])
            out.append({"index": int(m["index"]), "client_mac": _mac(mac), "yiaddr": _ip(m["yiaddr"]),
                        "lease_time": int(m["lease_time"]) if fl & abi.DHCP_HAS_LEASE_TIME else None,
                        "server_id": _ip(m["server_id"]) if fl & abi.DHCP_HAS_SERVER_ID else None,
                        "host_name": names.get(mac)})
    return out


def fingerprints(msgs, options, values) -> list[dict]:
    """Per DHCPv4 DISCOVER / REQUEST, in source order: the source packet, client_mac, msg_type, the option 55 list
    (None without the option) and the option 60 text, escaped (None without it). From the records of a call whose spec
    wanted options 55 and 60 with values."""
    values = bytes(values)
    out = []
    for m in msgs:
        if int(m["family"]) != 4 or int(m["msg_type"]) not in (DISCOVER, REQUEST):
            continue
        by = _by_code(m, options, values)
        vendor = by.get(60)
        out.append({"index": int(m["index"]), "client_mac": _mac(m["client_mac"]), "msg_type": int(m["msg_type"]),
                    "params": list(by[55]) if 55 in by else None,
                    "vendor": None if vendor is None else vendor.decode("latin-1").encode("unicode_escape").decode("ascii")})
    return out
