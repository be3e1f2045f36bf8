"""Slid packets for the parse's header windows (host only; tests/test_window_edges.py).

The tile kernel reads headers through an LDS window that ends p.lim = min(16 * nch - mis, caplen) bytes into the packet:
96 B in the one-round instances, 96 or 128 B after the first round and 144 B after the second round of the two-round
instances, minus the packet's address mod 16 (mod 4 after the dword-aligned re-gather). The window sizes are read from
the kernel source (window_constants), so the grid moves with them and the frozen fixture fails loudly when they change.

A slid packet is a header under test pushed across those edges by padding that adds few or no layer records: IPv4
options, an IPv6 hop-by-hop / destination-options extension, TCP options (in front of L7 bytes), GREv0 optional fields,
IPIP / 6in4 / 4in6 / GRE pairs and up to two VLAN tags. Padding moves the header in 4-byte steps; the 16 start
alignments every packet is placed at give the byte steps. For every kind of header (KINDS) the ladder of starts runs
from before the first edge minus the header's length to past the last edge, through paddings the fast path walks
(VLAN, MPLS, IPv4 options, one IPv6 extension, GRE) and paddings only the generic walk does (IPIP, 6in4, 4in6).

Other axes, pairwise: the capture ends a few bytes behind the last header or is padded to LONG bytes (only a long packet
can take the re-gather); the packets next to an edge are also cut at every byte from one before the header under test
to one past its end; five in eight packets carry valid IPv4 and L4 checksums (computed over the captured bytes, as the
engine sums them), the rest have one flipped bit in the L4 or the IPv4 checksum field. Three tile compositions
(COMPOSITIONS): only slid packets, slid packets alternating with plain Eth/IPv4/UDP|TCP ones, one slid packet among 63
plain ones.

Nothing here is seeded: the grid is a pure function of the window sizes.
"""
from __future__ import annotations

import re
import struct
from dataclasses import dataclass
from functools import lru_cache
from pathlib import Path

import numpy as np

import checksum_cases as cc
from pcapplusplus_amd import abi
from pcapplusplus_amd.pcap import PacketBatch

ROOT = Path(__file__).resolve().parents[1]
KERNELS = ROOT / "pcapplusplus_amd" / "csrc" / "pcppx_kernels.hip"
TILE = 64
LONG = 200          # captured bytes of a padded packet: (mis4 + caplen) >> 4 >= Chunks for every window up to 192 B
MAX_DESCRIPTORS = 60000
ALIGNS = tuple(range(16))


# ---------------------------------------------------------------- the windows, from the kernel source
@lru_cache(maxsize=None)
def window_constants() -> dict[str, int]:
    src = KERNELS.read_text()
    out = {}
    for name in ("kParseChunks", "kParseOnlyChunks", "kParseOnlyChunks1", "kParseDeepChunks1"):
        m = re.search(rf"\b{name}\s*=\s*(\d+)\s*[,;]", src)
        assert m, f"{name} not found in {KERNELS.name}"
        out[name] = int(m.group(1))
    return out


@dataclass(frozen=True)
class Instance:
    name: str
    csum: bool
    window: int
    first: int  # bytes of the first gather round
    full: int   # bytes of the whole window

    def opts(self, ml: int = 16, layout: int = abi.LAYOUT_FIXED) -> abi.Opts:
        return abi.make_opts(0, 8, self.csum, ml, self.window, layout)


@lru_cache(maxsize=None)
def instances() -> dict[str, Instance]:
    """The four product instances of parse_tile_kernel and the (checksums, window) that forces each."""
    k = window_constants()
    c, oc, oc1, dc1 = (16 * k[n] for n in ("kParseChunks", "kParseOnlyChunks", "kParseOnlyChunks1", "kParseDeepChunks1"))
    return {i.name: i for i in (Instance("csum", True, abi.WINDOW_SHORT, c, c),
                                Instance("csum_deep", True, abi.WINDOW_DEEP, dc1, oc),
                                Instance("only", False, abi.WINDOW_DEEP, oc1, oc),
                                Instance("only_short", False, abi.WINDOW_SHORT, c, c))}


@lru_cache(maxsize=None)
def edges() -> tuple[int, ...]:
    return tuple(sorted({e for i in instances().values() for e in (i.first, i.full)}))


def regather_edge() -> int:
    """The window the dword-aligned re-gather fills: the two-round instances' full window."""
    return instances()["only"].full


# ---------------------------------------------------------------- layer specs -> bytes
# A packet is a list of specs, outermost first; lengths, next-protocol fields and checksums are filled by assemble().
#   ("eth",) ("vlan",) ("mpls",) ("ip4", ihl[, frag]) ("ip6", ((ext type, bytes), ...)) ("gre0", c, k, s) ("gre1",)
#   ("ppp",) ("udp", sport, dport) ("tcp", sport, dport, doff) ("gtp", with extension chain) ("raw", tag, bytes)
GTP_EXT = b"\x00\x01\x00\x85" + bytes([1, 0x12, 0, 0x85]) + bytes([2, 1, 2, 3, 4, 5, 6, 0])  # seq, N-PDU, two extensions


def hdr_len(sp) -> int:
    t = sp[0]
    if t in ("eth", "vlan", "mpls", "ppp", "udp"):
        return {"eth": 14, "vlan": 4, "mpls": 4, "ppp": 4, "udp": 8}[t]
    if t == "ip4":
        return 4 * sp[1]
    if t == "ip6":
        return 40 + sum(n for _, n in sp[1])
    if t == "gre0":
        return 4 + 4 * (sp[1] + sp[2] + sp[3])
    if t == "gre1":
        return 16
    if t == "tcp":
        return 4 * sp[3]
    if t == "gtp":
        return 8 + (len(GTP_EXT) if sp[1] else 0)
    assert t == "raw", sp
    return len(sp[2])


def _ethertype(nxt, rest: int) -> int:
    if nxt is None:
        return 0x88B5
    t = nxt[0]
    if t == "raw":
        return {"arp": 0x0806, "llc": min(rest, 1500)}.get(nxt[1], 0x88B5)
    return {"vlan": 0x8100, "mpls": 0x8847, "ip4": 0x0800, "ip6": 0x86DD, "eth": 0x6558}[t]


def _ipproto(nxt) -> int:
    if nxt is None:
        return 253
    t = nxt[0]
    if t == "raw":
        return 1 if nxt[1] == "icmp" else 253
    return {"ip4": 4, "ip6": 41, "gre0": 47, "gre1": 47, "tcp": 6, "udp": 17}[t]


def _header(sp, nxt, rest: int, depth: int) -> bytes:
    """One header's bytes with its checksum fields zero; rest: the bytes behind it; depth: how many IP layers precede."""
    t = sp[0]
    if t == "eth":
        return cc.MAC_DST + cc.MAC_SRC + struct.pack(">H", _ethertype(nxt, rest))
    if t == "vlan":
        return struct.pack(">HH", 100 + depth, _ethertype(nxt, rest))
    if t == "mpls":
        return struct.pack(">I", 1000 << 12 | (0 if nxt is not None and nxt[0] == "mpls" else 1) << 8 | 64)
    if t == "ip4":
        ihl, frag = sp[1], (sp[2] if len(sp) > 2 else 0x4000)
        h = bytearray(b"\x01" * (4 * ihl))  # options: NOPs
        h[0], h[1] = 0x40 | ihl, 0
        struct.pack_into(">HHHBBH", h, 2, 4 * ihl + rest, 7 + depth, frag, 64, _ipproto(nxt), 0)
        h[12:16], h[16:20] = bytes([10, 1, 2, 3 + depth]), bytes([192, 168, 9, 1 + depth])
        return bytes(h)
    if t == "ip6":
        exts, body = sp[1], b""
        types = [e for e, _ in exts] + [_ipproto(nxt)]
        for k, (e, n) in enumerate(exts):
            if e == 44:    # fragment header: offset 0; M set when it is the last extension, else an atomic fragment
                assert n == 8
                body += bytes([types[k + 1], 0]) + struct.pack(">HI", 1 if k == len(exts) - 1 else 0, 0x01020304)
            elif e == 51:  # authentication header: length in dwords minus 2
                assert n % 4 == 0 and n >= 12
                body += bytes([types[k + 1], n // 4 - 2]) + b"\x00" * (n - 2)
            else:          # hop-by-hop 0, routing 43, destination options 60: length in 8-byte units minus 1
                assert n % 8 == 0 and 8 <= n <= 2048
                body += bytes([types[k + 1], n // 8 - 1]) + b"\x01" * (n - 2)
        src, dst = bytearray(cc.V6_SRC), bytearray(cc.V6_DST)
        src[15], dst[15] = (src[15] + depth) & 0xFF, (dst[15] + depth) & 0xFF
        return struct.pack(">IHBB", 0x60000000, len(body) + rest, types[0], 64) + bytes(src) + bytes(dst) + body
    if t == "gre0":
        c, k, s = sp[1:4]
        return bytes([c << 7 | k << 5 | s << 4, 0]) + struct.pack(">H", _ethertype(nxt, rest)) + b"\xaa" * (4 * (c + k + s))
    if t == "gre1":  # enhanced GRE (PPTP): K, S and A set, version 1, PPP behind it
        assert nxt is not None and nxt[0] == "ppp"
        return bytes([0x30, 0x81]) + struct.pack(">HHH", 0x880B, rest, 7) + b"\x00" * 8
    if t == "ppp":
        return bytes([0xFF, 0x03]) + struct.pack(">H", {"ip4": 0x21, "ip6": 0x57}[nxt[0]])
    if t == "udp":
        return struct.pack(">HHHH", sp[1], sp[2], 8 + rest, 0)
    if t == "tcp":
        h = bytearray(b"\x01" * (4 * sp[3]))  # options: NOPs
        struct.pack_into(">HHIIBBHHH", h, 0, sp[1], sp[2], 0x01020304, 0x05060708, sp[3] << 4, 0x18, 4096, 0, 0)
        return bytes(h)
    if t == "gtp":  # GTPv1-U G-PDU; with the E flag: sequence number, N-PDU number and two extension headers
        extra = GTP_EXT if sp[1] else b""
        return bytes([0x34 if sp[1] else 0x30, 0xFF]) + struct.pack(">HI", len(extra) + rest, 0x1234) + extra
    return sp[2]


def assemble(specs, cap: int | None = None, flip: str | None = None) -> bytes:
    """The packet's first `cap` bytes (None: all). Every IPv4 header and every TCP / UDP header that is captured whole
    then gets its valid checksum over the CAPTURED bytes (a cut L4 segment sums what is there, with the captured length
    in the pseudo header), innermost first. flip "l4": one bit of the innermost L4 checksum field is flipped before the
    outer sums are made (so only that verdict changes); flip "ip": one bit of the first IPv4 header's checksum."""
    lens = [hdr_len(s) for s in specs]
    offs = [sum(lens[:i]) for i in range(len(specs))]
    total = sum(lens)
    out, depth = bytearray(), 0
    for i, sp in enumerate(specs):
        out += _header(sp, specs[i + 1] if i + 1 < len(specs) else None, total - offs[i] - lens[i], depth)
        depth += sp[0] in ("ip4", "ip6")
    assert len(out) == total
    data = bytearray(out[:cap])
    n = len(data)
    ip4 = [i for i, sp in enumerate(specs) if sp[0] == "ip4" and offs[i] + lens[i] <= n]
    for i in ip4:
        struct.pack_into(">H", data, offs[i] + 10, cc.ipv4_header_checksum(bytes(data[offs[i]:offs[i] + lens[i]])))
    l4 = [i for i, sp in enumerate(specs) if sp[0] in ("tcp", "udp") and offs[i] + (20 if sp[0] == "tcp" else 8) <= n]
    for j, i in enumerate(reversed(l4)):
        ip = max(k for k in range(i) if specs[k][0] in ("ip4", "ip6"))
        o, proto = offs[ip], 6 if specs[i][0] == "tcp" else 17
        if specs[ip][0] == "ip4":
            ver, src, dst = 4, bytes(data[o + 12:o + 16]), bytes(data[o + 16:o + 20])
        else:
            ver, src, dst = 6, bytes(data[o + 8:o + 24]), bytes(data[o + 24:o + 40])
        at = offs[i] + (16 if proto == 6 else 6)
        c = cc.l4_checksum(ver, src, dst, proto, bytes(data[offs[i]:]))
        struct.pack_into(">H", data, at, c ^ (0x0100 if (flip == "l4" and j == 0) else 0))
    if flip == "ip" and ip4:
        data[offs[ip4[0]] + 11] ^= 0x04
    return bytes(data)


# ---------------------------------------------------------------- the headers under test
DATA = ("raw", "data", b"tail!")
UDP = ("udp", cc.SPORT, cc.DPORT)
TCP5 = ("tcp", cc.SPORT, cc.DPORT, 5)
V4_UDP = [("ip4", 5), UDP, DATA]
ARP = struct.pack(">HHBBH", 1, 0x0800, 6, 4, 1) + cc.MAC_SRC + bytes([10, 1, 2, 3]) + bytes(6) + bytes([10, 1, 2, 9])
ICMP_ECHO = bytes([8, 0, 0xF7, 0xFF, 0, 1, 0, 2]) + b"ping"
DNS = b"\x12\x34\x01\x00\x00\x01\x00\x00\x00\x00\x00\x00\x03www\x01a\x00\x00\x01\x00\x01"


@dataclass(frozen=True)
class Kind:
    """carrier: what names the header under test in the layer before it ("et" EtherType, "proto" IP protocol, "both").
    pre: fixed layers between the padding and the header under test (a UDP header before VXLAN, a VLAN tag before ARP; a
    TCP header's data offset None is padding too). hut: the header under test (first spec) and the stack behind it.
    h: its length, or the number of bytes the parse reads of it. proto: the pcppx protocol code of the layer record
    that starts at the header under test; whole: that record's hdr_len is h. v4_last: the padding must end in an IPv4
    or a GRE header (the reference builds neither IPv6 in IPv6 nor ICMP behind IPv6). lo: where the ladder starts, when
    that is lower than the first edge asks for."""
    name: str
    carrier: str
    pre: tuple
    hut: tuple
    h: int
    proto: int
    whole: bool = True
    v4_last: bool = False
    lo: int | None = None


def _kinds() -> list[Kind]:
    k = [
        Kind("vlan", "et", (), (("vlan",), *V4_UDP), 4, 9),
        Kind("mpls_bottom", "et", (("mpls",),), (("mpls",), *V4_UDP), 4, 14),
        Kind("arp", "et", (("vlan",),), (("raw", "arp", ARP),), 28, 8),
        Kind("llc", "et", (("vlan",),), (("raw", "llc", bytes([0xAA, 0xAA, 0x03]) + bytes(35)),), 3, 44),
        Kind("ipv4", "both", (), tuple(V4_UDP), 20, 2),
        Kind("ipv4_opts", "both", (), (("ip4", 9), TCP5, DATA), 36, 2),
        Kind("ipv4_mf", "both", (), (("ip4", 5, 0x2000), ("raw", "data", b"first fragment")), 20, 2),
        Kind("ipv4_offset", "both", (), (("ip4", 6, 0x0010), ("raw", "data", b"later fragment")), 24, 2),
        Kind("ipv6", "both", (), (("ip6", ()), TCP5, DATA), 40, 3, v4_last=True),
        Kind("ipv6_hop_dst", "both", (), (("ip6", ((0, 8), (60, 16))), UDP, DATA), 64, 3, v4_last=True),
        Kind("ipv6_dst_auth", "both", (), (("ip6", ((60, 8), (51, 24))), TCP5, DATA), 72, 3, v4_last=True),
        Kind("ipv6_frag", "both", (), (("ip6", ((44, 8),)), ("raw", "data", b"fragment")), 48, 3, v4_last=True),
        Kind("ipv6_rt_frag_dst", "both", (), (("ip6", ((43, 8), (44, 8), (60, 8))), UDP, DATA), 64, 3, v4_last=True),
        Kind("gre1_ppp", "proto", (), (("gre1",), ("ppp",), *V4_UDP), 16, 16),
        Kind("tcp_doff5", "proto", (), (TCP5, DATA), 20, 4),
        Kind("tcp_doff15", "proto", (), (("tcp", cc.SPORT, cc.DPORT, 15), DATA), 60, 4),
        Kind("udp", "proto", (), (UDP, DATA), 8, 5),
        Kind("udp_sip4", "proto", (), (UDP, ("raw", "data", b"INVITE sip:x")), 12, 5, whole=False),
        Kind("icmp_echo", "proto", (), (("raw", "icmp", ICMP_ECHO),), 8, 10, whole=False, v4_last=True),
        Kind("icmp_error_ipv4", "proto", (), (("raw", "icmp", bytes([3, 1, 0xFC, 0xFE, 0, 0, 0, 0])), ("ip4", 5), UDP),
             28, 10, whole=False, v4_last=True),
        Kind("vxlan", "proto", (("udp", 40000, 4789),), (("raw", "vxlan", bytes([8, 0, 0, 0, 0, 1, 2, 0])), ("eth",), *V4_UDP),
             8, 26),
        Kind("gtp", "proto", (("udp", 2152, 2152),), (("gtp", False), ("ip4", 5), TCP5, DATA), 8, 32),
        Kind("gtp_ext", "proto", (("udp", 2152, 2152),), (("gtp", True), ("ip4", 5), TCP5, DATA), 24, 32),
        Kind("http_request", "proto", (("tcp", 40000, 80, None),),
             (("raw", "data", b"GET /a HTTP/1.1\r\nHost: x\r\n\r\n"),), 17, 6, whole=False),
        Kind("http_response", "proto", (("tcp", 80, 40000, None),),
             (("raw", "data", b"HTTP/1.1 200 OK\r\nA: b\r\n\r\nbody"),), 17, 7, whole=False),
        Kind("ssl_record", "proto", (("tcp", 40000, 443, None),), (("raw", "data", bytes([22, 3, 1, 0, 5]) + b"hello"),), 5, 18, whole=False),
        Kind("dns", "proto", (("udp", 40000, 53),), (("raw", "data", DNS),), 12, 13, whole=False),
    ]
    for c in (0, 1):
        for key in (0, 1):
            for s in (0, 1):
                k.append(Kind(f"gre0_c{c}k{key}s{s}", "proto", (), (("gre0", c, key, s), *V4_UDP), 4 + 4 * (c + key + s), 15,
                              lo=34))  # from its natural offset: the whole GRE stack inside the 96-B window too
    return k


KINDS: dict[str, Kind] = {k.name: k for k in _kinds()}


# ---------------------------------------------------------------- padding
def _fill(r: int, parts, rot: int):
    """Counts for parts [(step, max)] that sum to r units, greedily in an order rotated by rot; None: impossible."""
    order = [(i + rot) % len(parts) for i in range(len(parts))]

    def go(j: int, left: int):
        if j == len(order):
            return {} if left == 0 else None
        step, hi = parts[order[j]]
        for c in range(min(hi, left // step), -1, -1):
            got = go(j + 1, left - c * step)
            if got is not None:
                got[order[j]] = c
                return got
        return None

    got = go(0, r)
    return None if got is None else [got[i] for i in range(len(parts))]


def _gre(g: int):
    return ("gre0", int(g >= 3), int(g >= 1), int(g >= 2))


def pad(flavor: str, via_gre: bool, length: int, v4_last: bool = False):
    """Specs of `length` bytes from the Ethernet header up to the header under test, or None.
    outer: Ethernet and up to two VLAN tags. fast4: Ethernet, VLAN tags, MPLS labels, IPv4 with options, GREv0 and a
    second IPv4 with options: a stack the fast path walks. v4: Ethernet, VLAN tags, IPv4 with options, then -- past 74 B, or on every
    other rung -- a second IPv4 (IPIP) or an IPv6 header (6in4). v6: Ethernet, at most one VLAN tag, IPv6 with a
    hop-by-hop or destination-options extension and, on every third rung, an IPv4 header with options (4in6).
    via_gre: a GREv0 header with 0-3 optional fields ends the padding (it names the header under test by EtherType).
    v4_last: no padding whose last header is IPv6 (6in4 is left out, v6 always ends in the 4in6 header or GRE)."""
    if length % 4 != 2:
        return None
    u, rot = (length - 14) // 4, length // 4
    gre = [(1, 3)] if via_gre else []
    g0 = 1 if via_gre else 0  # the GRE base header
    if flavor == "outer":
        return [("eth",)] + [("vlan",)] * u if (0 <= u <= 2 and not via_gre) else None
    if flavor == "fast4":
        # only bricks the fast path walks: VLAN tags, MPLS labels, IPv4 options and, where those do not reach, GREv0 with
        # an inner IPv4 header with options (a GRE header that carries the header under test stands alone)
        c = _fill(u - 5 - g0, [(1, 10), (1, 2), (1, 3)] + gre, rot)
        if c:
            return ([("eth",)] + [("vlan",)] * c[1] + [("mpls",)] * c[2] + [("ip4", 5 + c[0])] +
                    ([_gre(c[3])] if via_gre else []))
        c = None if via_gre else _fill(u - 5 - 1 - 5, [(1, 10), (1, 10), (1, 3), (1, 2), (1, 3)], rot)
        if c:
            return ([("eth",)] + [("vlan",)] * c[3] + [("mpls",)] * c[4] + [("ip4", 5 + c[0]), _gre(c[2]), ("ip4", 5 + c[1])])
        return None
    if flavor == "v4":
        shapes = ["pair", "single"] if (rot % 2 or length > 74) else ["single", "pair"]
        if rot % 5 == 0 and not (v4_last and not via_gre):
            shapes.insert(0, "6in4")
        for shape in shapes:
            if shape == "single":
                c = _fill(u - 5 - g0, [(1, 10)] + gre, rot)
                if c:
                    return [("eth",), ("ip4", 5 + c[0])] + ([_gre(c[1])] if via_gre else [])
            else:
                second = 10 if shape == "6in4" else 5
                c = _fill(u - 5 - second - g0, [(1, 10), (1, 10 if shape == "pair" else 0), (1, 2)] + gre, rot)
                if c:
                    inner = ("ip4", 5 + c[1]) if shape == "pair" else ("ip6", ())
                    return [("eth",)] + [("vlan",)] * c[2] + [("ip4", 5 + c[0]), inner] + ([_gre(c[3])] if via_gre else [])
        return None
    assert flavor == "v6"
    ext = 0 if rot % 2 else 60
    shapes = ["4in6", "plain"] if rot % 3 == 0 else ["plain", "4in6"]
    for shape in (["4in6"] if (v4_last and not via_gre) else shapes):
        tail = 5 if shape == "4in6" else 0
        c = _fill(u - 10 - 2 - tail - g0, [(2, 15), (1, 1), (1, 10 if tail else 0)] + gre, rot)
        if c:
            return ([("eth",)] + [("vlan",)] * c[1] + [("ip6", ((ext, 8 * (c[0] + 1)),))] +
                    ([("ip4", 5 + c[2])] if tail else []) + ([_gre(c[3])] if via_gre else []))
    return None


# ---------------------------------------------------------------- the grid
@dataclass(frozen=True)
class Slid:
    """One distinct packet of the grid."""
    kind: str
    flavor: str     # padding flavor, "+gre" where a GRE header carries the header under test
    s: int          # where the header under test starts
    h: int
    mode: str       # "built" | "long" | "cut"
    flip: str | None
    data: bytes
    aligns: tuple   # the start alignments this packet is placed at
    full_len: int   # the packet's length before a cut

    @property
    def caplen(self) -> int:
        return len(self.data)


def _stack(kind: Kind, flavor: str, via_gre: bool, s: int):
    """(specs, index of the header under test) with the header under test at byte s, or None."""
    for k in range(11):
        pre, fixed = list(kind.pre), 0
        for i, sp in enumerate(pre):
            if sp[0] == "tcp" and sp[3] is None:  # TCP options as padding: data offset 5-15, rotated by the rung
                pre[i] = (*sp[:3], 5 + (s // 4 + k) % 11)
            fixed += hdr_len(pre[i])
        front = pad(flavor, via_gre, s - fixed, kind.v4_last)
        if front is not None:
            return front + pre + list(kind.hut), len(front) + len(pre)
        if pre == list(kind.pre):
            break
    return None


def _lengthen(specs, to: int):
    total = sum(hdr_len(sp) for sp in specs)
    if total >= to:
        return specs
    fillb = bytes((0x61 + i % 26) for i in range(to - total))
    if specs[-1][0] == "raw" and specs[-1][1] in ("data", "llc", "icmp"):
        return specs[:-1] + [("raw", specs[-1][1], specs[-1][2] + fillb)]
    return specs + [("raw", "data", fillb)]


def _flavors(kind: Kind, rung: int):
    """(flavor, via_gre) pairs a rung of a kind's ladder is built through."""
    if kind.carrier == "et":
        return [("outer", False), ("v4" if rung % 2 else "fast4", True), ("v6", True)]
    if kind.carrier == "proto":
        return [("fast4", False), ("v4" if rung % 2 else "v6", False)]
    return [("outer", False)] + ([("fast4", True), ("v6", False)] if rung % 2 else [("v6", True), ("v4", False)])


def _flip(counter: int, has_l4: bool):
    if counter % 4 == 2:
        return "l4" if has_l4 else "ip"
    return "ip" if counter % 8 == 7 else None


@lru_cache(maxsize=None)
def grid() -> tuple[Slid, ...]:
    """Every distinct slid packet, in a fixed order (the fixture's row order)."""
    E = edges()
    out: list[Slid] = []
    counter = 0
    for kind in KINDS.values():
        lo = (E[0] - kind.h - 20) // 4 * 4 - 2  # 16 alignments reach back from the first feasible rung at or above it
        lo = lo if kind.lo is None else min(lo, kind.lo)
        near = {}  # edge -> the specs of the rung just before it (the cut packets)
        ladder = list(range(max(lo, 14), E[-1] + 3, 4))
        if kind.carrier != "proto":  # and outermost, behind 0-2 VLAN tags: no edge in reach, the first layer all the same
            ladder = [s for s in (14, 18, 22) if s < ladder[0]] + ladder
        for rung, s in enumerate(ladder):
            for flavor, via_gre in _flavors(kind, rung):
                st = _stack(kind, flavor, via_gre, s)
                if st is None:
                    continue
                specs, at = st
                assert sum(hdr_len(sp) for sp in specs[:at]) == s
                has_l4 = any(sp[0] in ("tcp", "udp") for sp in specs)
                modes = ["built", "long"] if s >= regather_edge() - kind.h - 8 else [("built", "long")[counter % 2]]
                for mode in modes:
                    sp = _lengthen(specs, LONG) if mode == "long" else specs
                    fl = _flip(counter, has_l4)
                    data = assemble(sp, None, fl)
                    out.append(Slid(kind.name, flavor + ("+gre" if via_gre else ""), s, kind.h, mode, fl, data,
                                    ALIGNS, len(data)))
                    counter += 1
                for e in E:
                    if e - 4 < s <= e and e not in near:
                        near[e] = (specs, flavor + ("+gre" if via_gre else ""), has_l4)
        # the rung next to each edge, cut at every byte from one before the header under test to one past its end; the
        # four alignments of a cut keep the header's start within 8 B of the edge (s - (e - mis) in -2..8)
        for n_e, (e, (specs, fname, has_l4)) in enumerate(sorted(near.items())):
            s = sum(hdr_len(sp) for sp in specs[:len(specs) - len(kind.hut)])
            full = sum(hdr_len(sp) for sp in specs)
            for c in range(-1, kind.h + 2):
                fl = _flip(counter, has_l4)
                data = assemble(_lengthen(specs, s + c), s + c, fl)
                aligns = tuple(sorted({(3 * c + 3 * j + n_e) % 11 for j in range(4)}))
                out.append(Slid(kind.name, fname, s, kind.h, "cut", fl, data, aligns, full))
                counter += 1
    return tuple(out)


# ---------------------------------------------------------------- placement and tile compositions
PLAIN = (assemble([("eth",), ("ip4", 5), UDP, ("raw", "data", b"a plain fast-path one")]),
         assemble([("eth",), ("ip4", 5), TCP5, ("raw", "data", b"and one over TCP")]))
COMPOSITIONS = ("solid", "mixed", "lone")


@dataclass
class Placed:
    name: str
    batch: PacketBatch
    uid: np.ndarray    # per descriptor: index into grid(), or -1 - j for plain packet j
    align: np.ndarray  # per descriptor: start address mod 16 (the buffer is 16-B aligned on the device)

    @property
    def slid(self) -> np.ndarray:
        return self.uid >= 0


@lru_cache(maxsize=None)
def _buffer():
    """One buffer for every composition: the two plain packets and every slid packet at each of its alignments, in
    cc.FILL bytes, 16 spare bytes at the end. Returns (data, {(uid, align): offset})."""
    items = [(-1 - j, a, p) for a in ALIGNS for j, p in enumerate(PLAIN)]
    items += [(u, a, sl.data) for u, sl in enumerate(grid()) for a in sl.aligns]
    where, pos, chunks = {}, 0, []
    for u, a, p in items:
        gap = (a - pos) % 16
        chunks.append(bytes([cc.FILL]) * gap)
        where[(u, a)] = pos + gap
        chunks.append(p)
        pos += gap + len(p)
    data = np.frombuffer(b"".join(chunks) + bytes([cc.FILL]) * 16, np.uint8).copy()
    return data, where


def _lone_pick(sl: Slid) -> bool:
    """The packets that get a tile of their own among 63 plain ones: the rung just before each edge (its alignment puts
    the header under test from 2 B before the edge to 13 B past it), and every eighth cut."""
    if sl.mode == "cut":
        return (sl.caplen - sl.s) % 8 == 0
    return any(sl.s == e - 2 for e in edges())


@lru_cache(maxsize=None)
def placed(name: str) -> Placed:
    data, where = _buffer()
    g = grid()
    desc: list[tuple[int, int]] = []
    plain = lambda j: (-1 - j % 2, (5 * j) % 16)  # noqa: E731  (alternating UDP / TCP, every alignment)
    if name == "solid":
        desc = [(u, a) for u, sl in enumerate(g) for a in sl.aligns]
    elif name == "mixed":
        for u, sl in enumerate(g):
            for a in sl.aligns:
                if (u + a) % 2 == 0:
                    desc += [(u, a), plain(len(desc))]
    else:
        assert name == "lone"
        for u, sl in enumerate(g):
            if _lone_pick(sl):
                a, at = sl.aligns[(7 * u) % len(sl.aligns)], (11 * u) % TILE
                tile = [plain(len(desc) + j) for j in range(TILE)]
                tile[at] = (u, a)
                desc += tile
    assert 0 < len(desc) <= MAX_DESCRIPTORS, (name, len(desc))
    uid = np.array([u for u, _ in desc], np.int32)
    align = np.array([a for _, a in desc], np.uint8)
    offs = np.array([where[d] for d in desc], np.uint64)
    caps = np.array([len(g[u].data) if u >= 0 else len(PLAIN[-1 - u]) for u, _ in desc], np.uint32)
    assert ((offs % 16) == align).all()
    return Placed(name, PacketBatch(data, offs, caps), uid, align)


def distinct_batch() -> PacketBatch:
    """The grid's distinct packets back to back (the frozen fixture's batch), the plain packets last."""
    from pcapplusplus_amd.pcap import from_packets

    return from_packets([sl.data for sl in grid()] + list(PLAIN))


def fixture_rows(uid: np.ndarray) -> np.ndarray:
    """Rows of distinct_batch() for the descriptors of a composition."""
    n = len(grid())
    return np.where(uid >= 0, uid, n + (-1 - uid)).astype(np.int64)
