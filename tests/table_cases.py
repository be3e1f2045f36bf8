"""A model of the open-addressed tables of pcppx_defrag.hip and pcppx_tcpstream.hip, keys crafted with it, and the
cases built from those keys (tests/test_group_tables.py).

The model restates how a key finds its slot: slots = max(64, the power of two >= 2 * room), the home slot from the
high bits of key * 0x9E3779B1, a linear probe that wraps at the last slot; tcpstream's segment table hashes
sid * 0x85EBCA6B + rel first. It is plain Python and numpy and only aims inputs: keys_at() inverts the multiplier, so a
case can put any number of keys on one home slot, next to the table's end, or on a solid run of slots. What a case must
give never comes from here: it comes from brute() and run_reference() of defrag_cases.py, defrag6_cases.py and
tcpstream_cases.py, whose builders the cases below are made with (those modules are imported inside the builders; the
model itself needs neither the oracle nor a GPU).

StandIn is slot_of() restated over a numpy array, the lanes of a wave in lockstep, with three switchable faults; it is
what shows that the cases' key sets would catch a wrong probe loop.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

M32 = 0xFFFFFFFF
MULT = 0x9E3779B1      # slot_of(): the home slot is (key * MULT) >> shift
SEG_MULT = 0x85EBCA6B  # seg_hash(): sid * SEG_MULT + rel is hashed as a key is
MINV = pow(MULT, -1, 1 << 32)
MIN_SLOTS = 64         # kDefragMinSlots, kTcpsMinSlots
CAND_PER_BLOCK = 256   # kDefragCandPerBlock, kTcpsCandPerBlock: the per-candidate kernels' block
OCCUPIED = 1 << 32


# ------------------------------------------------------------------ the model
def room_for(n: int, max_items: int) -> int:
    """defrag_room / tcpstream_room."""
    return n if max_items == 0 or max_items > n else max_items


def slots_for(room: int) -> int:
    """defrag_slots / tcpstream_slots."""
    c = MIN_SLOTS
    while c < 0x80000000 and c < 2 * room:
        c <<= 1
    return c


def shift_of(slots: int) -> int:
    assert slots & (slots - 1) == 0
    return 32 - (slots.bit_length() - 1)


def home(key: int, slots: int) -> int:
    return ((key * MULT) & M32) >> shift_of(slots)


def seg_home(sid: int, rel: int, slots: int) -> int:
    return home((sid * SEG_MULT + rel) & M32, slots)


def keys_at(home_slot: int, slots: int, count: int) -> list[int]:
    """count distinct 32-bit keys whose home is home_slot (home_slot 0: the first one is key 0)."""
    sh = shift_of(slots)
    assert 0 <= home_slot < slots and count <= 1 << sh
    keys = [(((home_slot << sh) + j) * MINV) & M32 for j in range(count)]
    assert all(home(k, slots) == home_slot for k in keys[:4] + keys[-4:])
    return keys


@dataclass
class Layout:
    occupied: frozenset      # the same for every insertion order
    displacement: int        # the longest one, for the order given
    wrapped: bool            # a key rests below its home
    where: dict              # key -> slot, for the order given


def layout(keys, slots: int, home_of=None) -> Layout:
    """Linear probing of the distinct keys in the order given. home_of: the home slot of a key that is no 32-bit key
    (the segment table's (sid, rel))."""
    nxt = list(range(slots))  # the next free slot at or behind s (path-compressed)

    def free_from(s: int) -> int:
        path = []
        while nxt[s] != s:
            path.append(s)
            s = nxt[s]
        for p in path:
            nxt[p] = s
        return s

    where: dict[int, int] = {}
    longest, wrapped = 0, False
    for k in keys:
        k = int(k) if home_of is None else k
        if k in where:
            continue
        assert len(where) < slots
        h = home(k, slots) if home_of is None else home_of(k)
        s = free_from(h)
        where[k] = s
        nxt[s] = (s + 1) & (slots - 1)
        longest = max(longest, (s - h) & (slots - 1))
        wrapped = wrapped or s < h
    return Layout(frozenset(where.values()), longest, wrapped, where)


# ------------------------------------------------------------------ slot_of() over a numpy array
FAULTS = ("no_mask", "lost_cas_claims", "stop_at_mismatch")


class StandIn:
    """slot_of<true> / slot_of<false> over an array of 64-bit words. insert_wave() steps up to 64 lanes in lockstep:
    all of them load, then those that saw a free slot compare-and-swap in lane order, so all but one of them lose.
    fault: "no_mask" drops the & (slots - 1) (the array has as many guard words behind it), "lost_cas_claims" takes a
    lost compare-and-swap for a claim, "stop_at_mismatch" ends a lookup at the first other key."""

    def __init__(self, slots: int, fault: str | None = None):
        assert fault is None or fault in FAULTS
        self.slots, self.fault = slots, fault
        self.words = np.zeros(2 * slots, np.uint64)

    def _next(self, s: int) -> int:
        return s + 1 if self.fault == "no_mask" else (s + 1) & (self.slots - 1)

    def insert_wave(self, keys) -> list:
        keys = [int(k) for k in keys]
        assert len(keys) <= 64
        s = [home(k, self.slots) for k in keys]
        got: list = [None] * len(keys)
        active = list(range(len(keys)))
        for _ in range(self.slots):
            seen = [int(self.words[s[ln]]) for ln in active]
            still = []
            for ln, k in zip(active, seen):
                want = OCCUPIED | keys[ln]
                if k == 0:
                    k = int(self.words[s[ln]])  # what the compare-and-swap returns
                    if k == 0:
                        self.words[s[ln]] = want
                    if k == 0 or self.fault == "lost_cas_claims":
                        got[ln] = s[ln]
                        continue
                if k == want:
                    got[ln] = s[ln]
                    continue
                s[ln] = self._next(s[ln])
                if s[ln] < len(self.words):
                    still.append(ln)
            active = still
        return got

    def lookup(self, key: int):
        want = OCCUPIED | int(key)
        s = home(int(key), self.slots)
        for _ in range(self.slots):
            k = int(self.words[s])
            if k == want:
                return s
            if k == 0 or self.fault == "stop_at_mismatch":
                return None
            s = self._next(s)
            if s >= len(self.words):
                return None
        return None


def check_standin(lanes, slots: int, absent=(), fault: str | None = None) -> None:
    """The key column `lanes` (one key per candidate, in batch order) inserted wave by wave, every key looked up
    again: each key has one slot inside the table and each slot one key, the slots are the model's, every key is found
    where it was put and the absent keys are not found."""
    t = StandIn(slots, fault)
    lanes = [int(k) for k in lanes]
    got = []
    for w in range(0, len(lanes), 64):
        got += t.insert_wave(lanes[w:w + 64])
    assert all(s is not None and s < slots for s in got), "a key without a slot of the table"
    by_key: dict[int, set] = {}
    by_slot: dict[int, set] = {}
    for k, s in zip(lanes, got):
        by_key.setdefault(k, set()).add(s)
        by_slot.setdefault(s, set()).add(k)
    assert all(len(v) == 1 for v in by_key.values()), "a key split over two slots"
    assert all(len(v) == 1 for v in by_slot.values()), "two keys in one slot"
    assert frozenset(by_slot) == layout(lanes, slots).occupied, "not the slots of linear probing"
    assert int(np.count_nonzero(t.words[slots:])) == 0
    for k, v in by_key.items():
        assert t.lookup(k) == next(iter(v)), "a key is not found where it was put"
    for k in absent:
        assert int(k) not in by_key and t.lookup(k) is None, "an absent key was found"


# ------------------------------------------------------------------ defrag / defrag6: the group table
STEP_EDGES = (32, 33, 64, 65, 1024, 1025)  # candidates = room on both sides of each doubling of slots
DENSE_N = 4096


def _aim_groups(c, key_of_id: dict[int, int]) -> None:
    """Every fragment of the case gets its group's crafted key (ip_key is an input column)."""
    from pcapplusplus_amd import abi

    for i in np.nonzero(c.info["ip_status"] & 15 == abi.IPR_FRAGMENT)[0]:
        c.info["ip_key"][i] = key_of_id[int(c.info["frag_id"][i])]


def _group_case(name: str, keys, sizes=None, n=None, places=None, extra=None, v6_every: int = 0, crafted=None,
                kind: str = "", **kw):
    """One group per key: clean groups of the given sizes (default: two members), crafted[j] the ready-made
    fragments of group j instead. v6_every: every v6_every-th clean group is an IPv6 one. max_fragments defaults to
    the candidate count: the smallest table."""
    import defrag6_cases as d6
    import defrag_cases as dc

    rng = np.random.default_rng([77, len(keys), v6_every])
    groups, ids = [], {}
    for j, key in enumerate(keys):
        ident = j + 1  # frag_id: the group's number
        ids[ident] = int(key)
        if crafted and j in crafted:
            groups.append(crafted[j](ident))
            continue
        sz = sizes(j) if sizes else [8, 3 + j % 6]
        if v6_every and j % v6_every == 1:
            groups.append(d6.group6(rng, ident, sz, src=0x100 + j))
        else:
            groups.append(dc.group(rng, ident, sz, src=0x0A000100 + j))
    ncand = sum(len(g) for g in groups)
    kw.setdefault("max_fragments", ncand)
    c = dc.make(name, dc.spread(rng, groups, ncand if n is None else n, places, extra), **kw)
    _aim_groups(c, ids)
    room = room_for(c.n, c.max_fragments)
    c.meta.update(keys=[int(k) for k in keys], slots=slots_for(room),
                  candidates=ncand, kind=kind)
    return c


def group_table_cases(v6_every: int = 0) -> list:
    """The crafted cases of the group table, as defrag cases; v6_every: with IPv6 groups in the same chains (for
    pcppx_defrag6_device with families V4 | V6). meta: keys (the groups' keys), slots, candidates, kind."""
    import defrag_cases as dc

    out = []
    mk = lambda *a, **kw: out.append(_group_case(*a, v6_every=v6_every, **kw))  # noqa: E731
    S = 128  # 64 candidates
    mk("one_home", keys_at(40, S, 32), kind="one_home")
    mk("wrap", keys_at(S - 6, S, 32), kind="wrap")
    mk("home_last_slot", keys_at(S - 1, S, 32), kind="wrap")
    # key 0 (home 0) behind a chain that has wrapped over slot 0: the chain's groups in the first tile, key 0's members
    # in the same wave's next one, so they come to a slot 0 that is taken
    chain = keys_at(S - 6, S, 31)
    places = [[2 * j, 2 * j + 1] for j in range(31)] + [[64, 65]]
    mk("key0_displaced", chain + [0], n=66, places=places, kind="key0")
    for room in STEP_EDGES:
        s = slots_for(room)
        three = (lambda j: [8, 8, 5] if j == 0 else [8, 3 + j % 6]) if room % 2 else None
        mk(f"step_{room}", keys_at(s - 3, s, room // 2), sizes=three, kind="step")
        assert out[-1].meta["candidates"] == room == out[-1].n
    # dense: every packet a candidate, no max_fragments: all keys at one home, then a solid run of homes with one key
    # more on its first slot, whose members come last in the batch
    s = slots_for(DENSE_N)
    mk("dense_one_home", keys_at(s - 6, s, DENSE_N // 2), max_fragments=0, kind="dense_one_home")
    run = [keys_at((s - 1000 + h) & (s - 1), s, 1)[0] for h in range(DENSE_N // 2 - 1)]
    collider = keys_at(s - 1000, s, 2)[1]
    perm = np.random.default_rng(5).permutation(DENSE_N - 2).reshape(-1, 2)
    places = [sorted(int(x) for x in p) for p in perm] + [[DENSE_N - 2, DENSE_N - 1]]
    mk("dense_run", run + [collider], places=places, max_fragments=0, kind="dense_run")
    # race: 8 groups of 8 interleaved in one tile, all keys at one home; and their members in 8 different blocks
    eight = lambda j: [8] * 7 + [3 + j]  # noqa: E731
    mk("race_tile", keys_at(S - 6, S, 8), sizes=eight, places=[[8 * m + g for m in range(8)] for g in range(8)],
       kind="race")
    mk("race_blocks", keys_at(S - 6, S, 8), sizes=eight, n=8 * dc.BLOCK, max_fragments=64,
       places=[[m * dc.BLOCK + 64 * g + m for m in range(8)] for g in range(8)], kind="race")
    # unclean groups mid-chain: their neighbours are still reassembled
    rng = np.random.default_rng(78)
    d = dc.udp_datagram(rng, 48)
    def fr(off, piece, more, ipid):
        return dc.eth() + dc.ipv4(0x0A000001, 0x0A000002, ipid, piece, foff=off, mf=more)

    crafted = {10: lambda ident: [fr(0, d[:16], True, ident), fr(24, d[24:], False, ident)],
               11: lambda ident: dc.group(rng, ident, dc.sizes_for(65, rng))}
    sc = slots_for(20 * 2 + 2 + 65)
    mk("unclean_in_chain", keys_at(sc - 9, sc, 22), crafted=crafted, kind="unclean",
       places=[list(range(2 * j, 2 * j + 2)) for j in range(10)] + [[20, 21], list(range(22, 87))]
       + [list(range(87 + 2 * j, 89 + 2 * j)) for j in range(10)])
    # all or nothing: the wrapped chain with room for one candidate less
    mk("overflow_in_chain", keys_at(S - 6, S, 32), max_fragments=63, kind="overflow")
    # a lone candidate whose home lies inside another key's wrapped chain (LEFT, found behind the chain), and a packet
    # the classifier leaves (FRAGMENT status, no IPv4 layer) under a key of the chain
    chain = keys_at(S - 6, S, 30)
    lone = keys_at(3, S, 1)[0]
    single = {30: lambda ident: [fr(0, d[:16], True, ident)]}
    places = [[2 * j, 2 * j + 1] for j in range(30)] + [[64]]
    c = _group_case("lookup_absent", chain + [lone], n=70, places=places, crafted=single, v6_every=v6_every,
                    extra={66: dc.eth(ethertype=0x0806) + bytes(28)}, kind="lookup_absent")
    from pcapplusplus_amd import abi

    c.info["ip_status"][66] = abi.IPR_FRAGMENT | abi.IPR_F_FIRST
    c.info["ip_key"][66] = chain[7]
    out.append(c)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def group_lanes(c) -> list[int]:
    """The key column of a group-table case's fragments, in batch order."""
    from pcapplusplus_amd import abi

    return [int(k) for k in c.info["ip_key"][c.info["ip_status"] & 15 == abi.IPR_FRAGMENT]]


# ------------------------------------------------------------------ tcpstream: the connection and the segment table
def _merge(rng, lists, n=None, places=None):
    """tcpstream_cases.interleave() (each list in its own order, fillers elsewhere) and, per packet, the list it came
    from (-1: a filler)."""
    import tcpstream_cases as tc

    total = sum(len(x) for x in lists)
    n = total if n is None else n
    if places is None:
        take = np.sort(rng.choice(n, total, replace=False))
        order = rng.permutation(np.repeat(np.arange(len(lists)), [len(x) for x in lists]))
        places = [[] for _ in lists]
        for t, li in zip(take, order):
            places[int(li)].append(int(t))
    owner = np.full(n, -1, np.int64)
    for li, pl in enumerate(places):
        owner[pl] = li
    return tc.interleave(rng, lists, n, places), owner


def _conn_case(name: str, keys, packets_of, n=None, places=None, kind: str = "", **kw):
    """One connection per key: packets_of(j, conn) its packets, in order. max_segments defaults to the candidate
    count."""
    import tcpstream_cases as tc

    rng = np.random.default_rng([79, len(keys)])
    lists = [packets_of(j, tc.Conn(j + 1, seed=31)) for j in range(len(keys))]
    ncand = sum(len(x) for x in lists)
    kw.setdefault("max_segments", ncand)
    pk, owner = _merge(rng, lists, n, places)
    c = tc.make(name, pk, **kw)
    for j, key in enumerate(keys):
        c.summary["hash5"][owner == j] = key  # an input column
    c.meta.update(keys=[int(k) for k in keys], slots=slots_for(room_for(c.n, c.max_segments)), candidates=ncand,
                  kind=kind, seg_words=[])
    return c


def _aimed_lengths(sid: int, start: int, count: int, target: int, slots: int) -> list[int]:
    """count segment lengths, each the shortest of 1..1400 whose end (the next segment's start) has the segment
    table's home `target`."""
    lens, at = [], start
    for _ in range(count):
        for ln in range(1, 1401):
            if seg_home(sid, at + ln, slots) == target:
                break
        else:
            raise LookupError(f"no length puts (sid {sid}, rel {at} + len) on slot {target} of {slots}")
        lens.append(ln)
        at += ln
    return lens


def _seg_case(name: str, target_of, edit=None, kind: str = "seg"):
    """One connection at its home slot: side 0 (sid = 2 * home) sends 26 data segments, the starts of all but the first
    and the end of the last on one home of the segment table; side 1 sends one. edit(packets): the batch changed."""
    import tcpstream_cases as tc

    conn = tc.Conn(501, seed=32)
    slots = MIN_SLOTS  # at most 28 candidates
    h = 9
    key = keys_at(h, slots, 1)[0]
    target = target_of(slots)
    lens = _aimed_lengths(2 * h, 0, 26, target, slots)
    side0 = conn.run(0, lens, syn=False, fin=False)
    pk = [side0[0], conn.pk(1, 1, 33)] + side0[1:]
    rels = [int(x) for x in np.cumsum([0] + lens[:-1])]
    if edit is not None:
        pk, rels = edit(pk, rels)
    c = tc.make(name, pk, max_segments=len(pk))
    c.summary["hash5"][:] = key
    assert slots_for(room_for(c.n, c.max_segments)) == slots
    c.meta.update(keys=[key], slots=slots, candidates=len(pk), kind=kind, seg_target=target,
                  seg_words=[(2 * h, r) for r in rels], seg_end=(2 * h, int(sum(lens))))
    return c


def _many_sides_case():
    """8 connections at 8 home slots, 9 data segments each, round robin: the starts of all but each side's first, 64
    words, on one home of the segment table. A home slot whose sid finds no length is passed over for the next one."""
    import tcpstream_cases as tc

    ncand = 72
    slots = slots_for(ncand)
    target = slots - 3
    lists, keys, words = [], [], []
    h = 5
    while len(lists) < 8:
        h += 1
        if h >= slots:
            raise LookupError("no eight home slots whose sides can be aimed")
        try:
            lens = _aimed_lengths(2 * h, 0, 9, target, slots)
        except LookupError:
            continue
        lists.append(tc.Conn(600 + len(lists), seed=33).run(0, lens, syn=False, fin=False))
        keys.append(keys_at(h, slots, 1)[0])
        words += [(2 * h, int(r)) for r in np.cumsum([0] + lens[:-1])]
    pk = [lists[i % 8][i // 8] for i in range(ncand)]
    c = tc.make("seg_many_sides", pk, max_segments=ncand)
    for i in range(ncand):
        c.summary["hash5"][i] = keys[i % 8]
    c.meta.update(keys=keys, slots=slots, candidates=ncand, kind="seg_many", seg_target=target, seg_words=words)
    return c


def stream_table_cases() -> list:
    """The crafted cases of tcpstream's two tables. meta: keys (the connections' hash5), slots, candidates, kind,
    seg_words ((sid, rel) of the data segments of the seg cases), seg_target."""
    import tcpstream_cases as tc

    out = []
    two = lambda j, c: [c.pk(0, 1, 10 + j % 7), c.pk(1, 1, 5 + j % 5)]  # one data segment per side  # noqa: E731
    mk = lambda name, keys, packets_of=two, **kw: out.append(_conn_case(name, keys, packets_of, **kw))  # noqa: E731
    S = 128
    mk("one_home", keys_at(40, S, 32), kind="one_home")
    mk("wrap", keys_at(S - 6, S, 32), kind="wrap")
    mk("home_last_slot", keys_at(S - 1, S, 32), kind="wrap")
    chain = keys_at(S - 6, S, 31)
    mk("key0_displaced", chain + [0], n=66, places=[[2 * j, 2 * j + 1] for j in range(31)] + [[64, 65]], kind="key0")
    for room in STEP_EDGES:
        s = slots_for(room)
        three = lambda j, c: two(j, c) + ([c.pk(0, 11 + j % 7, 4)] if j == 0 else [])  # noqa: E731
        mk(f"step_{room}", keys_at(s - 3, s, room // 2), three if room % 2 else two, kind="step")
        assert out[-1].meta["candidates"] == room == out[-1].n
    def four(j, c):  # two data segments per side
        return [c.pk(0, 1, 9 + j % 5), c.pk(1, 1, 6), c.pk(0, 10 + j % 5, 3), c.pk(1, 7, 2 + j % 9)]

    s = slots_for(DENSE_N)
    mk("dense_one_home", keys_at(s - 6, s, DENSE_N // 4), four, max_segments=0, kind="dense_one_home")
    run = [keys_at((s - 500 + h) & (s - 1), s, 1)[0] for h in range(DENSE_N // 4 - 1)]
    collider = keys_at(s - 500, s, 2)[1]
    perm = np.random.default_rng(6).permutation(DENSE_N - 4).reshape(-1, 4)
    places = [sorted(int(x) for x in p) for p in perm] + [list(range(DENSE_N - 4, DENSE_N))]
    mk("dense_run", run + [collider], four, places=places, max_segments=0, kind="dense_run")
    eight = lambda j, c: [p for m in range(4) for p in (c.pk(0, 1 + 5 * m, 5), c.pk(1, 1 + 3 * m, 3))]  # noqa: E731
    mk("race_tile", keys_at(S - 6, S, 8), eight, places=[[8 * m + g for m in range(8)] for g in range(8)], kind="race")
    mk("race_blocks", keys_at(S - 6, S, 8), eight, n=8 * tc.BLOCK, max_segments=64,
       places=[[m * tc.BLOCK + 64 * g + m for m in range(8)] for g in range(8)], kind="race")
    # the segment table
    out.append(_seg_case("seg_one_home", lambda s: 20))
    out.append(_seg_case("seg_wrap", lambda s: s - 3, kind="seg_wrap"))

    def swapped(pk, rels):
        pk = list(pk)
        pk[12], pk[13] = pk[13], pk[12]
        return pk, rels

    out.append(_seg_case("seg_ooo", lambda s: s - 3, swapped, kind="seg_wrap"))
    out.append(_seg_case("seg_duplicate", lambda s: s - 3, lambda pk, rels: (pk + [pk[-1]], rels), kind="seg_left"))
    out.append(_seg_case("seg_gap", lambda s: s - 3, lambda pk, rels: (pk[:13] + pk[14:], rels[:12] + rels[13:]),
                         kind="seg_left"))
    out.append(_many_sides_case())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def stream_lanes(c) -> list[int]:
    """The key column of a stream-table case's TCP packets, in batch order."""
    from pcapplusplus_amd import abi

    return [int(k) for k in c.summary["hash5"][c.info["tcp_status"] & 15 == abi.TCPR_DATA]]


def absent_keys(c) -> list[int]:
    """Keys that are not in the case's table and whose homes are the first three slots of its longest chain."""
    keys, slots = c.meta["keys"], c.meta["slots"]
    lay = layout(keys, slots)
    worst = max(lay.where, key=lambda k: (lay.where[k] - home(k, slots)) & (slots - 1))
    out = []
    for d in range(3):
        out.append(next(k for k in keys_at((home(worst, slots) + d) & (slots - 1), slots, len(keys) + 4)[::-1]
                        if k not in lay.where))
    return out

