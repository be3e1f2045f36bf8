"""Adversarial descriptor layouts for the host path's chunk staging (host only, no torch; tests/test_host_staging.py).

pcppx_parse_batch_host and pcppx_filter_batch_host cut a batch into chunks (stage_chunk / contiguous_chunk in
pcapplusplus_amd/csrc/pcppx_capi.cpp). A chunk is either copied straight from the caller's bytes ("direct": an ascending
run whose neighbours lie at most kMaxGap bytes apart, that ends the batch, is at least kMinRun packets long, or stops only
because the next ascending packet would not fit the chunk) or gathered packet by packet into pinned staging ("gather").

Two parts:
  plan()   a plain Python restatement of that decision, written from the comments and constants of pcppx_capi.cpp, so
           that a case can state which branch it was built to hit (the GPU tests cannot observe the branch);
  cases    builders that return a Case: the PacketBatch, the plan it must produce, and which descriptors are bad,
           oversize or empty. Packets are distinct real chains (checksum_cases.build) with the packet number stamped
           into the IPv4 identification and the source address, so that a record routed to the wrong packet cannot
           compare equal; `flows` builds the same layout over a small set of two-direction flows instead (the filter's
           flow table holds 4096 slots in these tests).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import checksum_cases as cc
from pcapplusplus_amd.pcap import PacketBatch

# the constants of pcppx_capi.cpp (test_host_staging.py::test_model_constants reads them out of the source)
K_MAX_GAP = 256
K_MIN_RUN = 4096
K_CHUNK_BYTES = 64 << 20
K_CHUNK_PACKETS = 1 << 18
MAX_CAPLEN = 65535  # PCPPX_MAX_CAPLEN: the kernels read no byte of a larger packet
M64 = (1 << 64) - 1

# why a run or a chunk stopped
GAP, OVERLAP, BELOW, BOUNDS, BYTES, PACKETS, END = "gap", "overlap", "below-run", "bounds", "bytes", "packets", "end"


# ---------------------------------------------------------------- the chunk-plan model
def _run(off, cap, n, data_len, i):
    """contiguous_chunk: (j, base, bytes, why) for the ascending run that starts at packet i."""
    end = base = off[i]
    j = i
    why = END
    while True:
        if j >= n:
            why = END
            break
        if j - i >= K_CHUNK_PACKETS:
            why = PACKETS
            break
        o, c = off[j], cap[j]
        if o < end:
            why = BELOW if o < base else OVERLAP
            break
        if o - end > K_MAX_GAP:
            why = GAP
            break
        if o + c > data_len:  # out of bounds, or an end that wraps 64 bits
            why = BOUNDS
            break
        if o + c - base > K_CHUNK_BYTES:
            why = BYTES
            break
        end = o + c
        j += 1
    return j, base, end - base, why


def explain(offsets, caplens, data_len):
    """The chunks of one host call: dicts {kind, i, j, staged, stop, run_stop}. stop: why the chunk ended; run_stop (a
    gathered chunk): why the run at its first packet was not taken directly."""
    off = [int(x) for x in np.asarray(offsets).tolist()]
    cap = [int(x) for x in np.asarray(caplens).tolist()]
    n = len(off)
    out = []
    i = 0
    while i < n:
        j, base, nbytes, why = _run(off, cap, n, data_len, i)
        # the third clause as the C code evaluates it: 64-bit unsigned arithmetic behind the `>= base` guard
        fits_not = j < n and off[j] >= base and ((off[j] + cap[j] - base) & M64) > K_CHUNK_BYTES
        if j > i and (j == n or j - i >= K_MIN_RUN or fits_not):
            out.append({"kind": "direct", "i": i, "j": j, "staged": nbytes, "stop": why})
            i = j
            continue
        pos = 0
        j = i
        stop = END
        while True:
            if j >= n:
                stop = END
                break
            if j - i >= K_CHUNK_PACKETS:
                stop = PACKETS
                break
            o, c = off[j], cap[j]
            take = c if (o + c <= data_len and c <= MAX_CAPLEN) else 0  # bad and oversize packets stage no bytes
            if pos + take > K_CHUNK_BYTES and j > i:
                stop = BYTES
                break
            pos += take
            j += 1
        out.append({"kind": "gather", "i": i, "j": j, "staged": pos, "stop": stop, "run_stop": why})
        i = j
    return out


def plan(offsets, caplens, data_len):
    """[(kind, i, j, staged_bytes)] with kind in {"direct", "gather"}: packets [i, j) per chunk, and the bytes copied
    to the device for it (a direct run's whole range, gaps included; a gathered chunk's packed packets)."""
    return [(c["kind"], c["i"], c["j"], c["staged"]) for c in explain(offsets, caplens, data_len)]


# ---------------------------------------------------------------- packets
@dataclass
class Case:
    name: str
    batch: PacketBatch
    plan: list                      # the plan the layout was built to produce
    bad: np.ndarray                 # descriptors the parse must flag PCPPX_F_BAD_DESC
    oversize: np.ndarray            # ... PCPPX_F_OVERSIZE
    empty: np.ndarray               # caplen 0
    max_layers: int = 12
    rich: bool = True               # at least 95% of the packets parse to three layers or more
    meta: dict = field(default_factory=dict)


FLOWS = 300          # flows of a `flows` build
HOT_FLOWS = 60       # of which this many share one endpoint address (the order-sensitive spec's src_ip)
HOT_ADDR = bytes([10, 77, 0, 1])


@lru_cache(maxsize=None)
def _templates(flows: bool) -> tuple:
    """S1 packets of 60-200 B: every family (IPv4 only for a `flows` build: the match spec reads IPv4 addresses)."""
    pk = [p for p in cc.s1_packets()[0] if 60 <= len(p.data) <= 200 and not (flows and not p.has_ip4)]
    return tuple(pk[:256])


def _flow_of(i: int) -> tuple[int, bool]:
    """(flow, reverse direction?) of packet i of a `flows` build: a fixed scramble, so that both directions of every
    flow occur all over the batch."""
    h = (i * 2654435761 + 12345) & 0xFFFFFFFF
    return (h >> 8) % FLOWS, bool((h >> 5) & 1) or (h >> 20) % 5 == 0


def stamp(p: cc.Pkt, i: int, flows: bool = False) -> bytes:
    """Packet i from template p. IPv4: the identification is i mod 2^16 and the source address 10.x.y.z holds i (the
    header checksum recomputed: IP_CSUM_OK); IPv6: the low four bytes of the source address hold i. flows: addresses and
    ports of flow _flow_of(i) instead. The L4 checksum is recomputed over the new pseudo header."""
    d = bytearray(p.data)
    v4 = p.has_ip4
    ip = 14
    proto = 6 if p.family.endswith("TCP") else 17
    if flows:
        f, rev = _flow_of(i)
        a = HOT_ADDR if f < HOT_FLOWS else bytes([10, 78, f >> 8, f & 0xFF])
        b = bytes([192, 168, 1 + (f >> 8), f & 0xFF])
        pa, pb = 20000 + f, 30000 + f % 7
        src, dst, sp, dp = (b, a, pb, pa) if rev else (a, b, pa, pb)
        d[ip + 12:ip + 16], d[ip + 16:ip + 20] = src, dst
        struct.pack_into(">HH", d, p.l4_off, sp, dp)
    elif v4:
        d[ip + 12:ip + 16] = bytes([10, (i >> 16) & 0xFF, (i >> 8) & 0xFF, i & 0xFF])
    else:
        d[ip + 8 + 12:ip + 8 + 16] = struct.pack(">I", i)
    if v4:
        struct.pack_into(">H", d, ip + 4, i & 0xFFFF)
        ihl = (d[ip] & 0xF) * 4
        struct.pack_into(">H", d, ip + 10, cc.ipv4_header_checksum(bytes(d[ip:ip + ihl])))
        src, dst = bytes(d[ip + 12:ip + 16]), bytes(d[ip + 16:ip + 20])
    else:
        src, dst = bytes(d[ip + 8:ip + 24]), bytes(d[ip + 24:ip + 40])
    at = p.l4_off + (16 if proto == 6 else 6)
    struct.pack_into(">H", d, at, cc.l4_checksum(4 if v4 else 6, src, dst, proto, bytes(d[p.l4_off:])))
    return bytes(d)


def packets(n: int, flows: bool = False, first: int = 0) -> list[bytes]:
    """n distinct stamped packets of 60-200 B, numbered from `first`."""
    t = _templates(flows)
    return [stamp(t[(first + k) % len(t)], first + k, flows) for k in range(n)]


@lru_cache(maxsize=None)
def _templates64() -> tuple:
    rng = np.random.default_rng(64)
    return (cc.build("IPv4/TCP", rng.bytes(10)), cc.build("IPv4/UDP", rng.bytes(22)), cc.build("IPv4/TCP", rng.bytes(10)),
            cc.build("IPv6/UDP", rng.bytes(2)))


def packets64(n: int, flows: bool = False) -> list[bytes]:
    """n distinct stamped packets of exactly 64 B."""
    t = _templates64()
    t = t[:3] if flows else t
    out = [stamp(t[k % len(t)], k, flows) for k in range(n)]
    assert all(len(p) == 64 for p in out[:8])
    return out


def lay(pkts: list[bytes], offsets: list[int], data_len: int | None = None, fill: int = cc.FILL) -> np.ndarray:
    """A buffer of `fill` bytes with the packets at their offsets; it ends with the last packet unless data_len says
    otherwise (a direct copy reads exactly the run, a gather exactly each packet)."""
    end = max((o + len(p) for o, p in zip(offsets, pkts)), default=0)
    data = np.full(max(end if data_len is None else data_len, 1), fill, dtype=np.uint8)
    for o, p in zip(offsets, pkts):
        data[o:o + len(p)] = np.frombuffer(p, dtype=np.uint8)
    return data


def packed_offsets(pkts: list[bytes], gap: int = 0, start: int = 0) -> list[int]:
    out, pos = [], start
    for p in pkts:
        out.append(pos)
        pos += len(p) + gap
    return out


def _none() -> np.ndarray:
    return np.zeros(0, dtype=np.int64)


def _case(name, data, offs, caps, plan_, bad=(), oversize=(), empty=(), **kw) -> Case:
    b = PacketBatch(data, np.asarray(offs, dtype=np.uint64), np.asarray(caps, dtype=np.uint32))
    ix = lambda v: np.asarray(sorted(v), dtype=np.int64)  # noqa: E731
    return Case(name, b, plan_, ix(bad), ix(oversize), ix(empty), **kw)


# ---------------------------------------------------------------- H1: the gap threshold
@lru_cache(maxsize=None)
def h1(gap: int, flows: bool = False) -> Case:
    pk = packets(5000, flows)
    offs = packed_offsets(pk, gap)
    total = sum(len(p) for p in pk)
    p = [("direct", 0, 5000, total + 4999 * gap)] if gap <= K_MAX_GAP else [("gather", 0, 5000, total)]
    return _case(f"H1 gap {gap}", lay(pk, offs), offs, [len(x) for x in pk], p)


def h1_slice(n: int) -> Case:
    """The first n packets of H1 (gap 0): one direct chunk."""
    c = h1(0)
    b = c.batch
    nbytes = int(b.caplens[:n].sum())
    return _case(f"H1 first {n}", b.data[:nbytes].copy(), b.offsets[:n].copy(), b.caplens[:n].copy(),
                 [("direct", 0, n, nbytes)])


# ---------------------------------------------------------------- H2: the run threshold
@lru_cache(maxsize=None)
def h2(run: int, flows: bool = False) -> Case:
    """Three ascending runs of `run` packets, a 1 KiB jump between runs."""
    pk = packets(3 * run, flows)
    offs, pos, sizes = [], 0, []
    for r in range(3):
        o = packed_offsets(pk[r * run:(r + 1) * run], 0, pos)
        offs += o
        sizes.append(o[-1] + len(pk[(r + 1) * run - 1]) - pos)
        pos = o[-1] + len(pk[(r + 1) * run - 1]) + 1024
    if run >= K_MIN_RUN:
        p = [("direct", r * run, (r + 1) * run, sizes[r]) for r in range(3)]
    else:  # the gather loop does not stop at the next run
        p = [("gather", 0, 3 * run, sum(sizes))]
    return _case(f"H2 runs of {run}", lay(pk, offs), offs, [len(x) for x in pk], p)


@lru_cache(maxsize=None)
def h2_tail() -> Case:
    """300 scattered packets, then a run of 100 that ends the batch: the gather that starts at packet 0 runs to the
    end of the batch, so the closing run is gathered with the rest (what the model says, pinned here)."""
    pk = packets(400)
    offs = packed_offsets(pk[:300], 700)
    offs += packed_offsets(pk[300:], 0, offs[-1] + len(pk[299]) + 700)
    return _case("H2 scattered then closing run", lay(pk, offs), offs, [len(x) for x in pk],
                 [("gather", 0, 400, sum(len(x) for x in pk))])


# ---------------------------------------------------------------- H3: many chunks, every slot reused
@lru_cache(maxsize=None)
def h3(flows: bool = False) -> Case:
    """Eight runs of 4096 x 64-B packets, each run at a lower address than the run before it: eight direct chunks."""
    run, nruns = K_MIN_RUN, 8
    pk = packets64(run * nruns, flows)
    offs = [((nruns - 1 - k // run) * run + k % run) * 64 for k in range(run * nruns)]
    p = [("direct", r * run, (r + 1) * run, run * 64) for r in range(nruns)]
    return _case("H3 eight descending runs", lay(pk, offs), offs, [64] * len(pk), p)


# ---------------------------------------------------------------- H4: unordered
@lru_cache(maxsize=None)
def h4(kind: str, flows: bool = False) -> Case:
    base = h1(0, flows).batch
    n = base.n
    total = int(base.caplens.sum())
    if kind in ("reversed", "global", "group64"):
        rng = np.random.default_rng(4)
        if kind == "reversed":
            perm = np.arange(n)[::-1]
        elif kind == "global":
            perm = rng.permutation(n)
        else:
            perm = np.concatenate([t0 + rng.permutation(min(64, n - t0)) for t0 in range(0, n, 64)])
        return _case(f"H4 {kind}", base.data, base.offsets[perm].copy(), base.caplens[perm].copy(),
                     [("gather", 0, n, total)])
    run = K_MIN_RUN
    if kind == "below":  # a direct run, then one packet below the run's base
        pk = packets(run + 1, flows)
        x = pk[run]
        offs = packed_offsets(pk[:run], 0, len(x) + 300) + [0]
        p = [("direct", 0, run, sum(len(q) for q in pk[:run])), ("direct", run, run + 1, len(x))]
        return _case("H4 run then a packet below it", lay(pk, offs), offs, [len(q) for q in pk], p)
    if kind == "below-short":  # the same with a run too short to be direct: only the `>= base` guard keeps it gathered
        pk = packets(100 + 1 + 200, flows)
        x = pk[100]
        offs = packed_offsets(pk[:100], 0, len(x) + 300) + [0]
        offs += packed_offsets(pk[101:], 0, offs[99] + len(pk[99]) + 2000)
        return _case("H4 short run then a packet below it", lay(pk, offs), offs, [len(q) for q in pk],
                     [("gather", 0, len(pk), sum(len(q) for q in pk))])
    assert kind == "below-run"  # run A, the packet below it, then run B contiguous with that packet
    pk = packets(2 * run + 1, flows)
    a, x, b = pk[:run], pk[run], pk[run + 1:]
    ob = packed_offsets(b, 0, len(x))
    oa = packed_offsets(a, 0, ob[-1] + len(b[-1]) + 300)
    offs = oa + [0] + ob
    p = [("direct", 0, run, sum(len(q) for q in a)), ("direct", run, 2 * run + 1, len(x) + sum(len(q) for q in b))]
    return _case("H4 run, a packet below it, a run behind that", lay(pk, offs), offs, [len(q) for q in pk], p)


# ---------------------------------------------------------------- H5: overlap
@lru_cache(maxsize=None)
def h5(kind: str, flows: bool = False) -> Case:
    if kind == "twice":  # every descriptor listed twice in a row
        pk = packets(2500, flows)
        offs = [o for o in packed_offsets(pk) for _ in (0, 1)]
        caps = [len(q) for q in pk for _ in (0, 1)]
        return _case("H5 every descriptor twice", lay(pk, offs[::2]), offs, caps, [("gather", 0, 5000, sum(caps))])
    if kind == "reach":  # caplens that reach 10 B into the next packet
        pk = packets(5000, flows)
        offs = packed_offsets(pk)
        caps = [len(q) + 10 for q in pk[:-1]] + [len(pk[-1])]
        return _case("H5 caplens reaching into the next packet", lay(pk, offs), offs, caps,
                     [("gather", 0, 5000, sum(caps))])
    assert kind == "same"
    pk = packets(3, flows)
    offs = packed_offsets(pk)
    return _case("H5 one packet 5000 times", lay(pk, offs), [offs[1]] * 5000, [len(pk[1])] * 5000,
                 [("gather", 0, 5000, 5000 * len(pk[1]))])


# ---------------------------------------------------------------- H6: bad descriptors inside a run
@lru_cache(maxsize=None)
def h6(first_bad: bool = True, flows: bool = False) -> Case:
    """A run of 9000 with out-of-bounds descriptors at 0 (first_bad), 4500 (its end wraps 64 bits) and 8999; the last
    good packet ends exactly at data_len. A bad first descriptor starts no run, so the gather takes the whole batch.
    Without it, and with a descriptor at 4500 that starts where the run goes on but runs past the buffer, the run is
    direct up to 4500 (it stops on the bounds check) and the rest is gathered."""
    n = 9000
    bad = ([0] if first_bad else []) + [4500, 8999]
    pk = packets(n, flows)
    good = [k for k in range(n) if k not in bad]
    go = packed_offsets([pk[k] for k in good])
    data = lay([pk[k] for k in good], go)
    data_len = len(data)
    assert go[-1] + len(pk[good[-1]]) == data_len
    offs, caps = [0] * n, [len(q) for q in pk]
    for k, o in zip(good, go):
        offs[k] = o
    offs[0] = data_len - 10 if first_bad else offs[0]  # starts inside the buffer, ends past it
    if first_bad:
        offs[4500] = (1 << 64) - 8                      # offset + caplen wraps 64 bits
    else:
        offs[4500], caps[4500] = offs[4501], data_len   # continues the run, but runs past the buffer
    offs[8999] = data_len - len(pk[8999]) + 1           # ends one byte past the buffer
    total = sum(len(pk[k]) for k in good)
    if first_bad:
        p = [("gather", 0, n, total)]
    else:
        head = sum(len(pk[k]) for k in range(4500))
        p = [("direct", 0, 4500, head), ("gather", 4500, n, total - head)]
    return _case("H6 bad descriptors" + ("" if first_bad else ", good first"), data, offs, caps, p, bad=bad,
                 rich=False)


# ---------------------------------------------------------------- H7: empty packets
@lru_cache(maxsize=None)
def h7(kind: str) -> Case:
    if kind == "middle":  # 5000 packets of caplen 0 in the middle of a run
        pk = packets(10000)
        o1 = packed_offsets(pk[:5000])
        mid = o1[-1] + len(pk[4999])
        o2 = packed_offsets(pk[5000:], 0, mid)
        offs = o1 + [mid] * 5000 + o2
        caps = [len(q) for q in pk[:5000]] + [0] * 5000 + [len(q) for q in pk[5000:]]
        total = sum(caps)
        return _case("H7 empty packets inside a run", lay(pk, o1 + o2), offs, caps, [("direct", 0, 15000, total)],
                     empty=range(5000, 10000), rich=False)
    assert kind == "all"  # every packet empty, at an offset below data_len: a direct chunk of zero bytes
    data = np.full(64, cc.FILL, dtype=np.uint8)
    return _case("H7 only empty packets", data, [10] * 5000, [0] * 5000, [("direct", 0, 5000, 0)], empty=range(5000),
                 rich=False)


# ---------------------------------------------------------------- H8: the chunk limits
H8A_N = 2 * K_CHUNK_PACKETS + 5


@lru_cache(maxsize=1)
def h8a(kind: str) -> Case:
    """2 * 2^18 + 5 contiguous Ethernet frames of 14-20 B (an unknown EtherType and 0-6 B behind it; the packet number
    in the source MAC), max_layers 2. ascending: direct 2^18 | 2^18 | 5; reversed: the same split, gathered;
    scatter-first: one far packet in front makes the first chunk a gather that stops on the packet limit, and the run
    that is left (four packets) ends the batch: the one gather -> direct transition."""
    n = H8A_N
    caps = (14 + (np.arange(n) * 5 + 3) % 7).astype(np.uint32)
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(caps[:-1], dtype=np.uint64)
    total = int(caps.sum())
    data = np.full(total + 64, cc.FILL, dtype=np.uint8)
    o = offs.astype(np.int64)
    idx = np.arange(n)
    data[o + 0] = 2
    for k in range(1, 6):
        data[o + k] = 0x10 + k
    data[o + 6] = 2
    data[o + 7] = 0xEE
    for k in range(4):
        data[o + 8 + k] = (idx >> (8 * (3 - k))) & 0xFF
    data[o + 12], data[o + 13] = 0x90, 0x00
    kw = {"max_layers": 2, "rich": False}
    cp = K_CHUNK_PACKETS
    cut = [int(offs[cp]), int(offs[2 * cp]), total]
    if kind == "ascending":
        p = [("direct", 0, cp, cut[0]), ("direct", cp, 2 * cp, cut[1] - cut[0]), ("direct", 2 * cp, n, cut[2] - cut[1])]
        return _case("H8a packet limit, ascending", data[:total], offs, caps, p, **kw)
    if kind == "reversed":
        p = [("gather", 0, cp, total - int(offs[n - cp])), ("gather", cp, 2 * cp, int(offs[n - cp] - offs[n - 2 * cp])),
             ("gather", 2 * cp, n, int(offs[n - 2 * cp]))]
        return _case("H8a packet limit, reversed", data[:total], offs[::-1].copy(), caps[::-1].copy(), p, **kw)
    assert kind == "scatter-first"
    m = cp + 4  # the far packet and 2^18 - 1 packets of the run, then four more that end the batch
    far = total + 40
    data[far:far + 14] = data[0:14]
    data[far + 8:far + 12] = [0xFF, 0xFF, 0xFF, 0xFE]
    so = np.concatenate([[np.uint64(far)], offs[:m - 1]]).astype(np.uint64)
    sc = np.concatenate([[np.uint32(14)], caps[:m - 1]]).astype(np.uint32)
    p = [("gather", 0, cp, 14 + int(offs[cp - 1])), ("direct", cp, m, int(offs[m - 1] - offs[cp - 1]))]
    return _case("H8a a far packet, then the run", data, so, sc, p, **kw)


def _big_packet(i: int, caplen: int) -> bytes:
    """Eth / IPv4 / UDP with 32 payload bytes, stamped; the rest of caplen is trailer (zeros in the buffer)."""
    t = cc.build("IPv4/UDP", bytes(range(32)))
    assert caplen >= len(t.data)
    return stamp(t, i)


@lru_cache(maxsize=1)
def h8_bytes(kind: str) -> Case:
    """The byte limit with packets of caplen 65535 (1024 of them leave exactly 1024 B of a 64 MiB chunk free).
    b: 1030 back to back: direct 1024 | 6, the first chunk stopping only because packet 1024 would not fit (a run
    shorter than kMinRun); b-reversed: gathered 1024 | 6. c-fit: 1024 of them, one 1024-B packet and three more: the
    first chunk is 1025 packets and exactly 64 MiB; c-over: a 1025-B packet in its place: 1024 | 4."""
    big = MAX_CAPLEN
    if kind in ("b", "b-reversed"):
        caps = [big] * 1030
    else:
        caps = [big] * 1024 + [1024 if kind == "c-fit" else 1025] + [100, 120, 140]
    n = len(caps)
    offs = [0] * n
    for k in range(1, n):
        offs[k] = offs[k - 1] + caps[k - 1]
    total = offs[-1] + caps[-1]
    data = np.zeros(total, dtype=np.uint8)
    for k in range(n):
        h = np.frombuffer(_big_packet(k, caps[k]), dtype=np.uint8)
        data[offs[k]:offs[k] + len(h)] = h
    first = 1024 * big
    if kind == "b":
        p = [("direct", 0, 1024, first), ("direct", 1024, n, total - first)]
    elif kind == "b-reversed":
        offs, caps = offs[::-1], caps[::-1]
        p = [("gather", 0, 1024, first), ("gather", 1024, n, total - first)]
    elif kind == "c-fit":
        assert first + 1024 == K_CHUNK_BYTES
        p = [("direct", 0, 1025, K_CHUNK_BYTES), ("direct", 1025, n, total - K_CHUNK_BYTES)]
    else:
        assert kind == "c-over"
        p = [("direct", 0, 1024, first), ("direct", 1024, n, total - first)]
    return _case(f"H8{kind} byte limit", data, offs, caps, p)


# ---------------------------------------------------------------- H9: oversize
@lru_cache(maxsize=None)
def h9_run(reverse: bool = False) -> Case:
    """In-bounds caplens 65536 and 70000 inside a run of 5000 (reverse: the same batch gathered)."""
    pk = packets(5000)
    caps = [len(q) for q in pk]
    caps[2000], caps[3000] = 65536, 70000
    offs = [0] * 5000
    for k in range(1, 5000):
        offs[k] = offs[k - 1] + caps[k - 1]
    total = offs[-1] + caps[-1]
    data = lay(pk, offs, total)
    if reverse:
        staged = total - 65536 - 70000  # no byte of an oversize packet is staged
        return _case("H9 oversize packets, gathered", data, offs[::-1], caps[::-1], [("gather", 0, 5000, staged)],
                     oversize=[1999, 2999], rich=False)
    return _case("H9 oversize packets inside a run", data, offs, caps, [("direct", 0, 5000, total)],
                 oversize=[2000, 3000], rich=False)


@lru_cache(maxsize=1)
def h9_huge() -> Case:
    """One packet of 64 MiB + 1 between two groups of ten small packets: the first ten are a direct chunk (the run stops
    only because the next packet would not fit), the rest is gathered, the huge packet staging no bytes."""
    pk = packets(21)
    huge = K_CHUNK_BYTES + 1
    caps = [len(q) for q in pk]
    caps[10] = huge
    offs = [0] * 21
    for k in range(1, 21):
        offs[k] = offs[k - 1] + caps[k - 1]
    total = offs[-1] + caps[-1]
    data = np.zeros(total, dtype=np.uint8)  # zeros: the huge packet's pages are never touched
    for k in range(21):
        if k != 10:
            data[offs[k]:offs[k] + len(pk[k])] = np.frombuffer(pk[k], dtype=np.uint8)
    p = [("direct", 0, 10, sum(caps[:10])), ("gather", 10, 21, sum(caps[11:]))]
    return _case("H9 a packet above 64 MiB", data, offs, caps, p, oversize=[10], rich=False)


# ---------------------------------------------------------------- H10: mixed
@lru_cache(maxsize=None)
def h10(flows: bool = False) -> Case:
    """A direct run of 5000, 300 scattered packets, one bad descriptor, a run of 5000, a short tail that ends the batch:
    the first run is direct (it stops at a gap), and the gather that follows runs to the end of the batch."""
    n = 5000 + 300 + 1 + 5000 + 40
    pk = packets(n, flows)
    offs = packed_offsets(pk[:5000])
    end = lambda: offs[-1] + len(pk[len(offs) - 1])  # noqa: E731
    offs += packed_offsets(pk[5000:5300], 900, end() + 900)
    bad_at = 5300
    offs.append(0)  # patched below
    offs += packed_offsets(pk[5301:10301], 0, offs[5299] + len(pk[5299]) + 900)
    offs += packed_offsets(pk[10301:], 3, end() + 5000)
    caps = [len(q) for q in pk]
    good = [k for k in range(n) if k != bad_at]
    data = lay([pk[k] for k in good], [offs[k] for k in good])
    offs[bad_at] = len(data) - 20
    caps[bad_at] = 60
    head = sum(caps[:5000])
    p = [("direct", 0, 5000, head), ("gather", 5000, n, sum(caps[k] for k in good) - head)]
    return _case("H10 mixed", data, offs, caps, p, bad=[bad_at])


# ---------------------------------------------------------------- the case lists
def small_cases() -> list:
    """(id, thunk) of every case below a few MiB."""
    out = [(f"H1-gap{g}", lambda g=g: h1(g)) for g in (0, 255, 256, 257)]
    out += [(f"H2-run{r}", lambda r=r: h2(r)) for r in (4095, 4096, 4097)]
    out += [("H2-tail", h2_tail), ("H3", h3)]
    out += [(f"H4-{k}", lambda k=k: h4(k)) for k in ("reversed", "global", "group64", "below", "below-short", "below-run")]
    out += [(f"H5-{k}", lambda k=k: h5(k)) for k in ("twice", "reach", "same")]
    out += [("H6", h6), ("H6-good-first", lambda: h6(False))]
    out += [(f"H7-{k}", lambda k=k: h7(k)) for k in ("middle", "all")]
    out += [("H9-run", h9_run), ("H9-gathered", lambda: h9_run(True)), ("H10", h10)]
    return out


def big_cases() -> list:
    """(id, thunk) of the cases that hold up to 68 MiB of host bytes or half a million packets (one of each kind is
    cached at most)."""
    out = [(f"H8a-{k}", lambda k=k: h8a(k)) for k in ("ascending", "reversed", "scatter-first")]
    out += [(f"H8{k}", lambda k=k: h8_bytes(k)) for k in ("b", "b-reversed", "c-fit", "c-over")]
    out += [("H9-huge", h9_huge)]
    return out


def all_cases() -> list:
    return small_cases() + big_cases()


def filter_cases() -> list:
    """(id, thunk) of the `flows` builds the filter tests run, each at most 33k packets, in the order in which a second
    call on the same context takes the next one."""
    return [("H1-gap257", lambda: h1(257, True)), ("H2-run4095", lambda: h2(4095, True)),
            ("H2-run4096", lambda: h2(4096, True)), ("H3", lambda: h3(True)),
            ("H4-reversed", lambda: h4("reversed", True)), ("H4-below-run", lambda: h4("below-run", True)),
            ("H5-twice", lambda: h5("twice", True)), ("H5-reach", lambda: h5("reach", True)),
            ("H6", lambda: h6(True, True)), ("H6-good-first", lambda: h6(False, True)), ("H10", lambda: h10(True))]
