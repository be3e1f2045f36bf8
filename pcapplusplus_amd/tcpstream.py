"""TCP sessions and TcpReassembly in numpy / plain Python, beside pcppx_tcpstream_device (include/pcppx.h, tcpstream).

sessions() generates TCP connections as a packet batch: the input side of the operator's tests and benchmark.
candidates() applies the contract's candidate rule to a parsed batch. Reassembler restates
TcpReassembly::reassemblePacket (Packet++/src/TcpReassembly.cpp:81-486) with handleFinOrRst (:501-527),
checkOutOfOrderFragments (:529-719) and closeConnectionInternal (:726-753) as a streaming machine, with both
configuration switches (enableBaseBufferClearCondition, maxOutOfOrderFragments) and the "[N bytes missing]" markers: the
model pcppx_tcpstream_device's contract is tested against, and the host completion of the packets the device leaves
(complete_on_host).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .pcap import PacketBatch

P_IPV4, P_IPV6, P_TCP = 2, 3, 4  # pcpp::ProtocolType
M32 = 0xFFFFFFFF


def seq_lt(a: int, b: int) -> bool:
    """SEQ_LT (TcpReassembly.cpp:16): the difference as a signed 32-bit number."""
    return ((a - b) & M32) >= 0x80000000


def seq_gt(a: int, b: int) -> bool:
    return 0 < ((a - b) & M32) < 0x80000000


# ------------------------------------------------------------------ the candidate rule
@dataclass
class Segment:
    """One candidate of the contract: what pcppx_tcpstream_device takes from a packet."""
    idx: int
    key: int     # hash5
    src: bytes   # address family, the raw source port bytes, the source address
    seq: int
    len: int     # info.tcp_payload
    pay: int     # the payload's offset in the packet
    syn: bool
    fin: bool
    rst: bool


def candidates(batch: PacketBatch, records, layers, info, data_len: int | None = None):
    """Per packet: ("bad" | "not_tcp" | "host" | "left" | "cand", Segment or None), by the rule of include/pcppx.h.
    records: a summary or brief array; layers: [n, max_layers]."""
    out = []
    dl = len(batch.data) if data_len is None else data_len
    ml = layers.shape[1] if batch.n else 0
    for i in range(batch.n):
        off, cap = int(batch.offsets[i]), int(batch.caplens[i])
        if off + cap > dl:
            out.append(("bad", None))
            continue
        st = int(info["tcp_status"][i])
        if st & 15 == abi.TCPR_HOST:
            out.append(("host", None))
            continue
        if st & 15 != abi.TCPR_DATA:
            out.append(("not_tcp", None))
            continue
        nl, l4 = min(int(records["n_layers"][i]), ml), int(records["l4_layer"][i])
        ln = int(info["tcp_payload"][i])
        seg = None
        if l4 < nl and int(layers[i, l4]["proto"]) == P_TCP:
            t, h = int(layers[i, l4]["offset"]), int(layers[i, l4]["hdr_len"])
            ip = next((k for k in range(nl) if int(layers[i, k]["proto"]) in (P_IPV4, P_IPV6)), None)
            if t + 20 <= cap and t + h + ln <= cap and ip is not None:
                fam = 4 if int(layers[i, ip]["proto"]) == P_IPV4 else 6
                io = int(layers[i, ip]["offset"])
                if io + (16 if fam == 4 else 24) <= cap:
                    pk = batch.data[off:off + cap]
                    addr = pk[io + 12:io + 16] if fam == 4 else pk[io + 8:io + 24]
                    seg = Segment(i, int(records["hash5"][i]), bytes([fam]) + pk[t:t + 2].tobytes() + addr.tobytes(),
                                  int.from_bytes(pk[t + 4:t + 8].tobytes(), "big"), ln, t + h,
                                  bool(st & abi.TCPR_F_SYN), bool(st & abi.TCPR_F_FIN), bool(st & abi.TCPR_F_RST))
        out.append(("cand", seg) if seg is not None else ("left", None))
    return out


# ------------------------------------------------------------------ TcpReassembly::reassemblePacket as a machine
@dataclass
class _Side:
    src: bytes | None = None
    sequence: int = 0
    frags: list = field(default_factory=list)  # the out-of-order list: [sequence, payload]
    got_fin_rst: bool = False


@dataclass
class _Conn:
    sides: list = field(default_factory=lambda: [_Side(), _Side()])
    n_sides: int = 0
    prev_side: int = -1
    closed: bool = False


class Reassembler:
    """TcpReassembly with an OnMessageReady callback that records what it is given: messages[(key, side)] is the list
    of (bytes, missing byte count, trimmed) per callback, in order, and log the (key, side, bytes) of all callbacks in
    the order they were made. trimmed: only a part of a payload was delivered (:359-365, :608-615)."""

    def __init__(self, base_clear: bool = True, max_out_of_order: int = 0):
        self.base_clear, self.max_ooo = base_clear, max_out_of_order
        self.conns: dict[int, _Conn] = {}
        self.messages: dict[tuple[int, int], list] = {}
        self.log: list[tuple[int, int, bytes]] = []

    def stream(self, key: int, side: int) -> bytes:
        return b"".join(m[0] for m in self.messages.get((key, side), []))

    def sides_of(self, key: int):
        c = self.conns.get(key)
        return [] if c is None else [s.src for s in c.sides[:c.n_sides]]

    def _deliver(self, key, side, data: bytes, missing: int = 0, trimmed: bool = False) -> None:
        self.messages.setdefault((key, side), []).append((bytes(data), missing, trimmed))
        self.log.append((key, side, bytes(data)))

    def feed(self, key: int, src: bytes, seq: int, payload: bytes, syn: bool, fin: bool, rst: bool) -> str:
        n = len(payload)
        fin_or_rst = fin or rst
        if n == 0 and not syn and not fin_or_rst:  # :133
            return "no_data"
        c = self.conns.get(key)
        if c is None:
            c = self.conns[key] = _Conn()
        elif c.closed:  # :173
            return "closed_flow"
        first = False
        if c.n_sides == 0:  # :195
            side, first = 0, True
        elif c.n_sides == 1:
            side = 0 if c.sides[0].src == src else 1
            first = side == 1
        elif c.sides[0].src == src:
            side = 0
        elif c.sides[1].src == src:
            side = 1
        else:
            return "no_match"  # :244
        s = c.sides[side]
        if first:
            s.src = src
            c.n_sides += 1
        if s.got_fin_rst:  # :256
            if not c.sides[1 - side].got_fin_rst and rst:
                self._fin_or_rst(c, 1 - side, key, rst)
                return "fin_rst"
            return "closed_flow"
        if fin_or_rst and n == 0:  # :271
            self._fin_or_rst(c, side, key, rst)
            return "fin_rst"
        if (self.base_clear and not first and n > 0 and c.prev_side != -1 and c.prev_side != side
                and c.sides[c.prev_side].frags):  # :297
            self._check_out_of_order(c, c.prev_side, key, True)
        c.prev_side = side
        if first:  # :312
            s.sequence = (seq + n + (1 if syn else 0)) & M32
            if n:
                self._deliver(key, side, payload)
            if fin_or_rst:
                self._fin_or_rst(c, side, key, rst)
            return "handled"
        if seq_lt(seq, s.sequence):  # :340
            status = "retransmission"
            if seq_gt((seq + n) & M32, s.sequence):
                new_len = (s.sequence - seq) & M32
                s.sequence = (s.sequence + n - new_len) & M32
                self._deliver(key, side, payload[new_len:], trimmed=True)
                status = "handled"
            if fin_or_rst:
                self._fin_or_rst(c, side, key, rst)
            return status
        if seq == s.sequence:  # :382
            if n == 0:
                return "no_data"
            s.sequence = (s.sequence + n + (1 if syn else 0)) & M32
            self._deliver(key, side, payload)
            self._check_out_of_order(c, side, key, False)
            if fin_or_rst:
                self._fin_or_rst(c, side, key, rst)
            return "handled"
        if n == 0:  # :439
            return "no_data"
        s.frags.append([seq, bytes(payload)])  # :458
        if self.max_ooo > 0 and len(s.frags) > self.max_ooo:
            self._check_out_of_order(c, side, key, False)
        if fin_or_rst:
            self._fin_or_rst(c, side, key, rst)
        return "buffered"

    def _fin_or_rst(self, c: _Conn, side: int, key: int, rst: bool) -> None:  # :501
        s = c.sides[side]
        if s.got_fin_rst:
            return
        s.got_fin_rst = True
        if c.sides[1 - side].got_fin_rst:
            self.close(key)
            return
        self._check_out_of_order(c, side, key, True)
        if rst:
            self.close(key)

    def _check_out_of_order(self, c: _Conn, side: int, key: int, clean_whole: bool) -> None:  # :529
        s = c.sides[side]
        while True:
            found = True
            while found:  # :548: the fragments at or below the current sequence
                found = False
                k = 0
                while k < len(s.frags):
                    fseq, data = s.frags[k]
                    if fseq == s.sequence:
                        s.frags.pop(k)
                        s.sequence = (s.sequence + len(data)) & M32
                        self._deliver(key, side, data)
                        found = True
                        continue
                    if seq_lt(fseq, s.sequence):
                        s.frags.pop(k)
                        if seq_gt((fseq + len(data)) & M32, s.sequence):
                            new_len = (s.sequence - fseq) & M32
                            s.sequence = (s.sequence + len(data) - new_len) & M32
                            self._deliver(key, side, data[new_len:], trimmed=True)
                            found = True
                        continue
                    k += 1
            if not clean_whole and (self.max_ooo == 0 or len(s.frags) <= self.max_ooo):  # :640
                return
            if not s.frags:
                return
            best = 0  # :652: the closest fragment above the current sequence
            for k in range(1, len(s.frags)):
                if seq_lt(s.frags[k][0], s.frags[best][0]):
                    best = k
            fseq, data = s.frags.pop(best)
            missing = (fseq - s.sequence) & M32
            s.sequence = (fseq + len(data)) & M32
            self._deliver(key, side, b"[%d bytes missing]" % missing + data, missing)

    def close(self, key: int) -> None:  # closeConnectionInternal :726
        c = self.conns.get(key)
        if c is None or c.closed:
            return
        self._check_out_of_order(c, 0, key, True)
        self._check_out_of_order(c, 1, key, True)
        c.closed = True

    def close_all(self) -> None:  # closeAllConnections
        for key in list(self.conns):
            self.close(key)

    def feed_batch(self, batch: PacketBatch, records, layers, info, only=None) -> None:
        """Every candidate of the batch, in source order (only: a boolean mask of the packets to feed)."""
        for i, (kind, g) in enumerate(candidates(batch, records, layers, info)):
            if kind != "cand" or (only is not None and not only[i]):
                continue
            start = int(batch.offsets[i]) + g.pay
            self.feed(g.key, g.src, g.seq, batch.data[start:start + g.len].tobytes(), g.syn, g.fin, g.rst)


def complete_on_host(batch: PacketBatch, records, layers, info, disposition, base_clear: bool = True,
                     max_out_of_order: int = 0) -> Reassembler:
    """What a host caller does with pcppx_tcpstream_device's result: the packets the device LEFT go through
    TcpReassembly (here: its restatement) in source order. Returns the machine; its messages are the streams of the
    sides the device did not reassemble."""
    r = Reassembler(base_clear, max_out_of_order)
    r.feed_batch(batch, records, layers, info, only=np.asarray(disposition) == abi.TCPS_LEFT)
    return r


# ------------------------------------------------------------------ sessions
TH_FIN, TH_SYN, TH_RST, TH_PSH, TH_ACK = 1, 2, 4, 8, 16


@dataclass
class Sessions:
    batch: PacketBatch
    conn: np.ndarray     # per packet: the connection's number
    side: np.ndarray     # 0 = the client (the SYN's sender), 1 = the server
    seq: np.ndarray
    length: np.ndarray   # TCP payload bytes
    flags: np.ndarray    # TH_*
    extra: np.ndarray    # 0 = an original segment, 1 = a duplicate, 2 = a keep-alive
    pay_off: np.ndarray  # the payload's offset in the packet

    def plaintext(self, conn: int, side: int) -> bytes:
        """What the side sent: its original data segments in sequence order (lost ones included: they were dropped
        from the batch, and a side with a loss is not clean)."""
        return self._plain[(conn, side)]

    _plain: dict = field(default_factory=dict)


def sessions(connections: int, segments: int | tuple[int, int] = 6, mss: int = 1460, seed: int = 0,
             interleave: str = "mixed", reorder: float = 0.0, duplicate: float = 0.0, loss: float = 0.0,
             keepalive: float = 0.0, syn_data: float = 0.0, fin: str = "end", rst: float = 0.0, ipv6: float = 0.0,
             syn: bool = True, vlan: bool = False, min_len: int = 1, spread: float = 4.0) -> Sessions:
    """`connections` TCP connections, Ethernet [+ VLAN] + IPv4 / IPv6 + TCP, interleaved in one batch.
    segments: data segments per side (a number, or a (lo, hi) range drawn per side); mss: the largest payload (lengths
    are drawn from min_len..mss). interleave: "sequential" (the client's data, then the server's), "mixed" (both sides'
    data merged at random) -- the connections themselves overlap in time (spread: how many connections are in flight
    at once, roughly). reorder / duplicate / loss: the fraction of data segments that arrive a few packets late / twice
    / not at all (a side's last segment is never lost: a hole, not a shorter stream). keepalive: the fraction of sides
    that send a 1-byte keep-alive at their next sequence number - 1.
    syn_data: the fraction of connections whose SYN carries data. fin: "end" (a zero-length FIN behind each side's
    data), "data" (FIN on the last data segment), "early" (a zero-length FIN ahead of the side's last data segment),
    "none". rst: the fraction of connections whose server sends a RST, at a random place. ipv6: the fraction of
    connections over IPv6. syn = False: no handshake, the stream starts mid-flow.
    Payload bytes are random; plaintext(conn, side) gives what each side sent."""
    rng = np.random.default_rng(seed)
    lo, hi = (segments, segments) if isinstance(segments, int) else segments
    rows = []  # (time, conn, side, seq, len, flags, extra, origin row for a duplicate)
    plain_len = {}
    dt = 1.0
    for c in range(connections):
        t0 = float(rng.uniform(0, max(1.0, connections * (2 * hi + 4) / spread)))
        ks = [int(rng.integers(lo, hi + 1)) for _ in range(2)]
        isn = [int(rng.integers(0, 1 << 32)) for _ in range(2)]
        with_syn_data = syn and rng.random() < syn_data
        if interleave == "sequential":
            times = [2 + np.arange(ks[0], dtype=float), 2 + ks[0] + np.arange(ks[1], dtype=float)]
        else:
            slots = rng.permutation(ks[0] + ks[1])
            times = [2 + np.sort(slots[:ks[0]]).astype(float), 2 + np.sort(slots[ks[0]:]).astype(float)]
        end = 2 + ks[0] + ks[1]
        for d in range(2):
            nxt = isn[d]
            if syn:
                ln = int(rng.integers(1, 64)) if (with_syn_data and d == 0) else 0
                rows.append([t0 + d * dt * 0.5, c, d, nxt, ln, TH_SYN | (TH_ACK if d else 0), 0])
                nxt = (nxt + 1 + ln) & M32
            total = 0
            for j in range(ks[d]):
                ln = int(rng.integers(min_len, mss + 1))
                t = t0 + times[d][j] * dt
                fl = TH_ACK | (TH_PSH if j == ks[d] - 1 else 0)
                if fin == "data" and j == ks[d] - 1:
                    fl |= TH_FIN
                if rng.random() < reorder:
                    t += float(rng.uniform(1.5, 4.5)) * dt
                if rng.random() < loss and j < ks[d] - 1:  # never the last one: what is left would tile again
                    rows.append([-1.0, c, d, nxt, ln, fl, 0])  # dropped below; its bytes stay in the plaintext
                else:
                    rows.append([t, c, d, nxt, ln, fl, 0])
                    if rng.random() < duplicate:
                        rows.append([t + float(rng.uniform(0.5, 3.5)) * dt, c, d, nxt, ln, fl, 1])
                nxt = (nxt + ln) & M32
                total += ln
            plain_len[(c, d)] = total
            if rng.random() < keepalive:
                rows.append([t0 + (end + 0.25 + 0.1 * d) * dt, c, d, (nxt - 1) & M32, 1, TH_ACK, 2])
            if fin == "end":
                rows.append([t0 + (end + 1 + 0.5 * d) * dt, c, d, nxt, 0, TH_FIN | TH_ACK, 0])
            elif fin == "early" and ks[d] >= 2:
                rows.append([t0 + (times[d][-1] - 0.5) * dt, c, d, nxt, 0, TH_FIN | TH_ACK, 0])
        if rng.random() < rst:
            rows.append([t0 + float(rng.uniform(1.5, end + 1.5)) * dt, c, 1, isn[1], 0, TH_RST, 0])
    tab = np.array(rows, dtype=np.float64).reshape(-1, 7)
    # the plaintext: every original data segment's random bytes, in sequence order per side
    orig = tab[:, 6] == 0
    plain = {}
    seg_bytes = {}
    for r in np.nonzero(orig & (tab[:, 4] > 0))[0]:
        c, d, sq, ln = int(tab[r, 1]), int(tab[r, 2]), int(tab[r, 3]), int(tab[r, 4])
        b = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        seg_bytes[(c, d, sq)] = b
        plain[(c, d)] = plain.get((c, d), b"") + b
    keep = np.nonzero(tab[:, 0] >= 0)[0]
    keep = keep[np.argsort(tab[keep, 0], kind="stable")]
    v6 = rng.random(connections) < ipv6
    packets, pay_off = [], []
    for r in keep:
        c, d, sq, ln, fl, ex = (int(tab[r, k]) for k in range(1, 7))
        if ex == 2:
            body = b"\0"
        else:
            body = seg_bytes.get((c, d, sq), b"")[:ln] if ln else b""
        cp, sp = 20000 + c % 40000, 80 + c % 7
        sport, dport = (cp, sp) if d == 0 else (sp, cp)
        tcp = struct.pack(">HHIIBBHHH", sport, dport, sq, 0, 0x50, fl, 65535, 0, 0) + body
        ca, sa = 0x0A000000 + c, 0xC0A80000 + (c * 7) % 65536
        if v6[c]:
            a = [b"\x20\x01\x0d\xb8" + bytes(8) + struct.pack(">I", x) for x in (ca, sa)]
            ip = struct.pack(">IHBB", 0x60000000, len(tcp), 6, 64) + a[d] + a[1 - d]
            et = 0x86DD
        else:
            h = bytearray(struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(tcp), int(r) & 0xFFFF, 0x4000, 64, 6, 0,
                                      ca if d == 0 else sa, sa if d == 0 else ca))
            s = sum(struct.unpack(">10H", bytes(h)))
            while s >> 16:
                s = (s & 0xFFFF) + (s >> 16)
            h[10:12] = struct.pack(">H", ~s & 0xFFFF)
            ip, et = bytes(h), 0x0800
        l2 = bytes.fromhex("020000000001020000000002") + (struct.pack(">HHH", 0x8100, 100 + c % 50, et) if vlan
                                                          else struct.pack(">H", et))
        packets.append(l2 + ip + tcp)
        pay_off.append(len(l2) + len(ip) + 20)
    from .pcap import from_packets

    batch = from_packets(packets) if packets else PacketBatch(np.zeros(1, np.uint8), np.zeros(0, np.uint64),
                                                              np.zeros(0, np.uint32))
    col = lambda k, dt_: tab[keep, k].astype(dt_)  # noqa: E731
    for k in plain_len:
        plain.setdefault(k, b"")
    return Sessions(batch, col(1, np.uint32), col(2, np.uint8), col(3, np.uint64).astype(np.uint32),
                    col(4, np.uint32), col(5, np.uint8), col(6, np.uint8), np.array(pay_off, np.uint32), plain)


def session_batch(n: int, flows: int, seed: int = 4, sizes=(64, 576, 1500), weights=(0.55, 0.25, 0.20),
                  zipf: float = 1.1) -> tuple[PacketBatch, np.ndarray]:
    """A benchmark batch, built with numpy alone: n Ethernet + IPv4 + TCP packets with payload, their connections
    drawn from `flows` with a Zipf law (a few elephants of thousands of segments, many mice), the direction at random,
    every side's sequence numbers continuing in arrival order (no SYN: every side is clean and in order). Returns the
    batch and the per-packet side number (2 * flow + direction). Payload bytes are random."""
    rng = np.random.default_rng(seed)
    flow = np.minimum(rng.zipf(zipf, n) - 1, flows - 1).astype(np.int64) if flows > 1 else np.zeros(n, np.int64)
    flow = (flow * 2654435761 % flows).astype(np.int64)  # the elephants spread over the address space
    side = rng.integers(0, 2, n).astype(np.int64)
    size = rng.choice(np.asarray(sizes), n, p=np.asarray(weights)).astype(np.int64)
    pay = size - 54
    assert (pay > 0).all()
    fs = flow * 2 + side
    order = np.argsort(fs, kind="stable")
    csum = np.cumsum(pay[order]) - pay[order]
    first = np.r_[True, fs[order][1:] != fs[order][:-1]]
    base = np.maximum.accumulate(np.where(first, csum, 0))
    rel = np.empty(n, np.int64)
    rel[order] = csum - base
    isn = (fs * 0x9E3779B1 + 12345) & M32
    seq = ((isn + rel) & M32).astype(np.uint32)
    offsets = (np.cumsum(size) - size).astype(np.uint64)
    data = rng.integers(0, 256, int(size.sum()), dtype=np.uint8)
    hdr = np.zeros((n, 54), np.uint8)
    hdr[:, 0:12] = np.frombuffer(bytes.fromhex("020000000001020000000002"), np.uint8)
    hdr[:, 12], hdr[:, 13] = 0x08, 0x00
    be = lambda a, w: np.stack([(a >> (8 * (w - 1 - k))) & 0xFF for k in range(w)], axis=1).astype(np.uint8)  # noqa
    ca, sa = 0x0A000000 + flow, 0xC0A80000 + (flow * 7) % 65536 + ((flow // 65536) << 16)
    cp, sp = 1024 + flow % 60000, 80 + flow % 7
    hdr[:, 14], hdr[:, 22], hdr[:, 23] = 0x45, 64, 6
    hdr[:, 16:18] = be(size - 14, 2)
    hdr[:, 20] = 0x40
    hdr[:, 26:30] = be(np.where(side == 0, ca, sa), 4)
    hdr[:, 30:34] = be(np.where(side == 0, sa, ca), 4)
    words = hdr[:, 14:34].astype(np.uint32)
    s = (words[:, 0::2] << 8 | words[:, 1::2]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    hdr[:, 24:26] = be((~s) & 0xFFFF, 2)
    hdr[:, 34:36] = be(np.where(side == 0, cp, sp), 2)
    hdr[:, 36:38] = be(np.where(side == 0, sp, cp), 2)
    hdr[:, 38:42] = be(seq.astype(np.int64), 4)
    hdr[:, 46], hdr[:, 47] = 0x50, TH_ACK
    hdr[:, 48:50] = 0xFF
    data[(offsets[:, None].astype(np.int64) + np.arange(54)[None, :]).reshape(-1)] = hdr.reshape(-1)
    return PacketBatch(data, offsets, size.astype(np.uint32)), fs


__all__ = [n for n in dir() if not n.startswith("_")]
