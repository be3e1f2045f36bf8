"""Cases and an independent reference for pcppx_bpf_device / pcppx_bpf_reference (tests/test_bpf.py).

interp() is a plain per-packet Python loop written from the machine semantics stated in include/pcppx.h (bpf), not
from the C++: Python integers never wrap, so every modulo-2^32 step and every bound is spelled out here. cases() builds
the families the kernel can go wrong on: batch shapes (tile edges, base alignments, gapped and unordered batches, the
caplens around the load sizes, bad descriptors), the edges of every load, the ALU edges, all 16 M[] slots, control flow
(a 64-way divergent tile, a 4096-instruction program, long jumps), several programs, and a seeded fuzz.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from pcapplusplus_amd import abi, bpf
from pcapplusplus_amd.bpf import (ABS, ADD, ALU, AND, DIV, IMM, IND, JA, JEQ, JGE, JGT, JMP, JSET, LD, LDX, LEN, LSH,
                                  MEM, MISC, MOD, MSH, MUL, NEG, OR, RET, RSH, ST, STX, SUB, TAX, TXA, XOR, A, B, H, K,
                                  W, X, insn)

FILL = 0xA5
PAD = 64          # entries of every output column past n: they must keep FILL
M32 = 0xFFFFFFFF
COLUMNS = ("matched", "bucket", "ret")
SIZE = {W: 4, H: 2, B: 1}


# ---------------------------------------------------------------- the independent interpreter
def run_one(prog: list[tuple[int, int, int, int]], pkt: bytes, wirelen: int) -> tuple[int, int, bool]:
    """One program over one packet: (the return value, instructions executed, ended by an out-of-bounds load)."""
    a = x = 0
    mem = [0] * 16
    buflen = len(pkt)
    pc = steps = 0
    while True:
        code, jt, jf, k = prog[pc]
        pc += 1
        steps += 1
        cls = code & 0x07
        if cls in (LD, LDX):
            mode = code & 0xE0
            if mode == IMM:
                v = k
            elif mode == MEM:
                v = mem[k]
            elif mode == LEN:
                v = wirelen
            else:
                size = SIZE[code & 0x18]
                xx = x if mode == IND else 0
                if k > buflen or xx > buflen - k or size > buflen - (xx + k):
                    return 0, steps, True
                v = int.from_bytes(pkt[xx + k: xx + k + size], "big")
                if mode == MSH:
                    v = (v & 0xF) << 2
            if cls == LDX:
                x = v
            else:
                a = v
        elif cls == ST:
            mem[k] = a
        elif cls == STX:
            mem[k] = x
        elif cls == ALU:
            s = x if code & 0x08 else k
            op = code & 0xF0
            if op == ADD:
                a = (a + s) & M32
            elif op == SUB:
                a = (a - s) & M32
            elif op == MUL:
                a = (a * s) & M32
            elif op in (DIV, MOD):
                if s == 0:
                    return 0, steps, False
                a = a // s if op == DIV else a % s
            elif op == OR:
                a |= s
            elif op == AND:
                a &= s
            elif op == XOR:
                a ^= s
            elif op == LSH:
                a = (a << s) & M32 if s < 32 else 0
            elif op == RSH:
                a = a >> s if s < 32 else 0
            else:
                assert op == NEG
                a = (-a) & M32
        elif cls == JMP:
            s = x if code & 0x08 else k
            op = code & 0xF0
            if op == JA:
                pc += k
            else:
                t = {JEQ: a == s, JGT: a > s, JGE: a >= s, JSET: (a & s) != 0}[op]
                pc += jt if t else jf
        elif cls == RET:
            return (a if (code & 0x18) == A else k), steps, False
        else:
            assert cls == MISC
            if (code & 0xF8) == TXA:
                a = x
            else:
                x = a


# ---------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    data: np.ndarray          # u8: the batch's buffer
    offsets: np.ndarray       # u64[n]
    caplens: np.ndarray       # u32[n]
    programs: list            # of bpf.INSN_DTYPE arrays, in load order
    frame_lens: np.ndarray | None = None
    data_len: int | None = None   # None: len(data)
    misalign: int = 0         # the device buffer starts this many bytes past a 16-B boundary
    columns: tuple = COLUMNS  # the non-NULL output columns

    @property
    def n(self) -> int:
        return len(self.offsets)

    def dlen(self) -> int:
        return len(self.data) if self.data_len is None else self.data_len


@dataclass
class Result:
    matched: np.ndarray  # u8[n + PAD]
    bucket: np.ndarray   # u8[n + PAD]
    ret: np.ndarray      # u32[n + PAD]
    totals: np.ndarray   # u64[8]
    stats: dict = field(default_factory=dict)


def blank(n: int) -> Result:
    return Result(np.full(n + PAD, FILL, np.uint8), np.full(n + PAD, FILL, np.uint8),
                  np.full(n + PAD, FILL * 0x01010101, np.uint32), np.full(abi.BPF_TOTALS, FILL, np.uint64))


def interp(case: Case) -> Result:
    """The contract by the Python interpreter: the columns the case asks for, FILL elsewhere."""
    out = blank(case.n)
    progs = [p.tolist() for p in case.programs]
    raw = case.data.tobytes()
    dl = case.dlen()
    matched_n = bad = steps4 = oob = pairs = 0
    for i in range(case.n):
        off, cap = int(case.offsets[i]), int(case.caplens[i])
        m, bk, rv = 0, 0xFF, 0
        if off + cap > dl:  # Python integers: the 64-bit wrap is out of bounds as well
            bad += 1
        else:
            pkt = raw[off: off + cap]
            wl = cap if case.frame_lens is None else int(case.frame_lens[i])
            for q, p in enumerate(progs):
                r, steps, was_oob = run_one(p, pkt, wl)
                pairs += 1
                steps4 += steps >= 4
                oob += was_oob
                if r != 0:
                    m, bk, rv = 1, q, r
                    break
            matched_n += m
        if "matched" in case.columns:
            out.matched[i] = m
        if "bucket" in case.columns:
            out.bucket[i] = bk
        if "ret" in case.columns:
            out.ret[i] = rv
    out.totals[:] = 0
    out.totals[abi.BPF_MATCHED] = matched_n
    out.totals[abi.BPF_BAD_DESC] = bad
    out.stats = {"pairs": pairs, "accepted": matched_n, "oob": oob, "steps4": steps4}
    return out


def c_batch(case: Case) -> abi.Batch:
    return abi.Batch(case.data.ctypes.data, case.offsets.ctypes.data, case.caplens.ctypes.data, case.dlen(), case.n,
                     abi.LINKTYPE_ETHERNET, 0)


def verdicts(res: Result, columns) -> abi.BpfVerdicts:
    col = lambda name, a: abi.ptr(a) if name in columns else None  # noqa: E731
    return abi.BpfVerdicts(col("matched", res.matched), col("bucket", res.bucket), col("ret", res.ret),
                           abi.ptr(res.totals))


def run_reference(case: Case) -> Result:
    """pcppx_bpf_reference over the case (host pointers)."""
    out = blank(case.n)
    fl = None if case.frame_lens is None else case.frame_lens.ctypes.data
    abi.bpf_reference(case.programs, c_batch(case), fl, verdicts(out, case.columns))
    return out


def run_device(engine, case: Case, dev: str = "cuda:0", source=None, stream=None, flt=None) -> Result:
    """pcppx_bpf_device over the case. source: (data, offsets, caplens, data_len) device tensors to use instead of an
    upload of the case's own (the wide source); flt: programs already loaded (else the case's are, and freed)."""
    import torch

    n = case.n
    if source is None:
        raw = torch.zeros(len(case.data) + 32, dtype=torch.uint8, device=dev)
        lead = (case.misalign - raw.data_ptr()) % 16
        data = raw[lead: lead + len(case.data)]
        data.copy_(torch.from_numpy(case.data))
        assert data.data_ptr() % 16 == case.misalign
        offs = torch.from_numpy(case.offsets.view(np.int64)).to(dev)
        caps = torch.from_numpy(case.caplens.view(np.int32)).to(dev)
        dl = case.dlen()
    else:
        data, offs, caps, dl = source
    fl = None if case.frame_lens is None else torch.from_numpy(case.frame_lens.view(np.int32)).to(dev)
    host = blank(n)
    t = {k: torch.from_numpy(getattr(host, k).view(np.int32 if k == "ret" else np.uint8)).to(dev) for k in COLUMNS}
    totals = torch.from_numpy(host.totals.view(np.int64)).to(dev)
    col = lambda k: t[k] if k in case.columns else None  # noqa: E731
    own = flt is None
    if own:
        flt = engine.bpf_load(case.programs)
    try:
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(st):
            engine.bpf_device(flt, data, offs, caps, n, abi.LINKTYPE_ETHERNET, totals, col("matched"), col("bucket"),
                              col("ret"), fl, st.cuda_stream, data_len=dl)
        st.synchronize()
    finally:
        if own:
            flt.free()
    return Result(t["matched"].cpu().numpy(), t["bucket"].cpu().numpy(), t["ret"].cpu().numpy().view(np.uint32),
                  totals.cpu().numpy().view(np.uint64))


def assert_same(got: Result, want: Result, what: str) -> None:
    """Every column whole (the FILL past n and of a NULL column included) and the totals."""
    for k in COLUMNS:
        g, w = getattr(got, k), getattr(want, k)
        if not np.array_equal(g, w):
            bad = np.nonzero(g != w)[0]
            raise AssertionError(f"{what}: {k} differs at {bad[:8].tolist()} ({len(bad)} entries): "
                                 f"got {g[bad[:8]].tolist()}, want {w[bad[:8]].tolist()}")
    assert got.totals.tolist() == want.totals.tolist(), (what, got.totals.tolist(), want.totals.tolist())


# ---------------------------------------------------------------- batches
def packed(lens, seed: int, lo: int = 0, hi: int = 256, lead: int = 0, tail: int = 0):
    """Packets of the given lengths, random bytes in [lo, hi), back to back after `lead` bytes."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.uint32)
    total = int(lens.sum(dtype=np.uint64))
    data = rng.integers(lo, hi, lead + total + tail, dtype=np.uint8)
    offs = (lead + np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)
    return data, offs, lens


def random_lens(n: int, seed: int, hi: int = 200) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, hi + 1, n).astype(np.uint32)


def prog(*rows) -> np.ndarray:
    return bpf.program(rows)


# a verdict that depends on several bytes of the packet: X = 4 * (P[0] & 15), A = be16 at X + 1, + X; accept on bit 0
P_MIX = prog(insn(LDX | B | MSH, k=0), insn(LD | H | IND, k=1), insn(ALU | ADD | X), insn(JMP | JSET | K, 0, 1, 1),
             insn(RET | A), insn(RET | K, k=0))
# the first and the last byte of the packet (wirelen = caplen): be8 first * 256 + last, + 1
P_ENDS = prog(insn(LD | W | LEN), insn(ALU | SUB | K, k=1), insn(MISC | TAX), insn(LD | B | IND, k=0), insn(ST, k=3),
              insn(LD | B | ABS, k=0), insn(ALU | LSH | K, k=8), insn(LDX | MEM, k=3), insn(ALU | ADD | X),
              insn(ALU | ADD | K, k=1), insn(RET | A))


def shape_cases() -> list[Case]:
    out = []
    for n in (0, 1, 63, 64, 65, 129, 1000):
        d, o, c = packed(random_lens(n, 100 + n), 200 + n)
        out.append(Case(f"n{n}", d, o, c, [P_MIX]))
    for mis in range(8):  # the device buffer's base, and with it every packet's address mod 4 and mod 8
        d, o, c = packed(random_lens(129, 300 + mis, 90), 310 + mis, lead=mis)
        out.append(Case(f"base{mis}", d, o, c, [P_ENDS], misalign=mis))
    # gapped and unordered: the packets of a packed batch, 0..9 bytes apart, descriptors shuffled
    rng = np.random.default_rng(7)
    lens = random_lens(200, 320, 120)
    gaps = rng.integers(0, 10, 200)
    offs = (np.cumsum(lens + gaps) - lens).astype(np.uint64)
    data = rng.integers(0, 256, int(offs[-1] + lens[-1]) + 5, dtype=np.uint8)
    order = rng.permutation(200)
    out.append(Case("gapped_unordered", data, offs[order].copy(), lens[order].astype(np.uint32), [P_ENDS]))
    # the caplens around the load sizes, an oversize packet, and the last packet ending exactly at data_len
    lens = np.array([0, 1, 3, 4, 70000, 2, 5, 0, 8, 7, 70000, 4, 1], np.uint32)
    d, o, c = packed(lens, 330)
    assert int(o[-1]) + int(c[-1]) == len(d)
    out.append(Case("caplens_0_1_3_4_70000", d, o, c, [P_ENDS]))
    out.append(Case("caplens_mix", d, o, c, [P_MIX]))
    # bad descriptors among live packets: one byte past data_len, at data_len, far past it, a 64-bit wrap; and the
    # legal neighbours: ending exactly at data_len, an empty packet at data_len
    d, o, c = packed(random_lens(130, 340, 80) + 1, 341)
    dl = len(d)
    o, c = o.copy(), c.copy()
    for i, (off, cap) in {3: (dl - 10, 11), 64: (dl, 1), 65: (dl + (1 << 32), 4), 70: (0xFFFFFFFFFFFFFFF0, 64),
                          71: (0xFFFFFFFFFFFFFFFF, 1), 100: (dl - 10, 10), 101: (dl, 0), 129: (1 << 63, 0)}.items():
        o[i], c[i] = off, cap
    out.append(Case("bad_desc", d, o, c, [P_ENDS]))
    out.append(Case("bad_desc_two_programs", d, o, c, [prog(insn(RET | K, k=0)), P_MIX]))
    return out


def load_edge_cases() -> list[Case]:
    """k fixed, the caplens run through it: caplen = k - 1 .. k + size + 1 puts k at caplen - size - 1 .. caplen + 1.
    Bytes are 1..255, so a load that succeeds returns non-zero."""
    out = []
    k = 21
    lens = np.repeat(np.arange(0, 41, dtype=np.uint32), 4)  # four packets per caplen: the addresses differ mod 4
    d, o, c = packed(lens, 400, lo=1)
    for sz, nm in ((W, "w"), (H, "h"), (B, "b")):
        out.append(Case(f"abs_{nm}", d, o, c, [prog(insn(LD | sz | ABS, k=k), insn(RET | A))]))
        out.append(Case(f"abs_{nm}_k0", d, o, c, [prog(insn(LD | sz | ABS, k=0), insn(RET | A))]))
        # the same position as X + k, split three ways
        for xv, kk in ((0, k), (k, 0), (7, k - 7)):
            out.append(Case(f"ind_{nm}_x{xv}", d, o, c,
                            [prog(insn(LDX | IMM, k=xv), insn(LD | sz | IND, k=kk), insn(RET | A))]))
        # X = caplen (one past the last byte); X = caplen - size through LEN: the last value that fits
        out.append(Case(f"ind_{nm}_x_caplen", d, o, c,
                        [prog(insn(LDX | W | LEN), insn(LD | sz | IND, k=0), insn(RET | A))]))
        out.append(Case(f"ind_{nm}_last", d, o, c,
                        [prog(insn(LD | W | LEN), insn(ALU | SUB | K, k=SIZE[sz]), insn(MISC | TAX),
                              insn(LD | sz | IND, k=0), insn(RET | A))]))
        # nothing wraps 32 bits: X + k = 2^32 + 1, k alone past the packet, X alone past it
        out.append(Case(f"ind_{nm}_wrap", d, o, c,
                        [prog(insn(LDX | IMM, k=M32), insn(LD | sz | IND, k=2), insn(RET | K, k=9))]))
        out.append(Case(f"ind_{nm}_kmax", d, o, c,
                        [prog(insn(LDX | IMM, k=0), insn(LD | sz | IND, k=M32), insn(RET | K, k=9))]))
        out.append(Case(f"ind_{nm}_kmax_x2", d, o, c,
                        [prog(insn(LDX | IMM, k=2), insn(LD | sz | IND, k=M32), insn(RET | K, k=9))]))
        out.append(Case(f"abs_{nm}_kmax", d, o, c, [prog(insn(LD | sz | ABS, k=M32), insn(RET | K, k=9))]))
    # MSH at the last byte (caplen = k + 1) and one past it (caplen = k)
    out.append(Case("msh", d, o, c, [prog(insn(LDX | B | MSH, k=k), insn(MISC | TXA), insn(ALU | ADD | K, k=1),
                                          insn(RET | A))]))
    out.append(Case("msh_kmax", d, o, c, [prog(insn(LDX | B | MSH, k=M32), insn(RET | K, k=9))]))
    return out


ACC = 15  # the M[] slot the ALU programs accumulate in


def accumulate(snippets) -> np.ndarray:
    """Each snippet leaves a value in A; M[ACC] = M[ACC] * 0x01000193 + A after each; the program returns M[ACC] | 1."""
    rows = []
    for s in snippets:
        rows += list(s)
        rows += [insn(MISC | TAX), insn(LD | MEM, k=ACC), insn(ALU | MUL | K, k=0x01000193), insn(ALU | ADD | X),
                 insn(ST, k=ACC)]
    rows += [insn(LD | MEM, k=ACC), insn(ALU | OR | K, k=1), insn(RET | A)]
    return bpf.program(rows)


def alu_cases() -> list[Case]:
    out = []
    d, o, c = packed(np.full(70, 12, np.uint32), 500)
    d[0:12] = 0                     # packet 0: all zero
    d[12:24] = 0xFF                 # packet 1: all ones
    d[24:28] = (0x80, 0, 0, 0)      # packet 2: the top bit alone
    d[36:40] = (0, 0, 0, 1)         # packet 3: the low bit alone
    ld = insn(LD | W | ABS, k=0)
    shifts = (0, 1, 31, 32, 33, 0x80000000, M32)
    ops = []
    for op in (LSH, RSH):
        for sh in shifts:  # through K, then through X
            ops.append((ld, insn(ALU | op | K, k=sh)))
            ops.append((insn(LDX | IMM, k=sh), ld, insn(ALU | op | X)))
    out.append(Case("alu_shifts", d, o, c, [accumulate(ops)]))
    ops = []
    for kk in (0, 1, 0x10001, 0x80000000, M32):
        for op in (ADD, SUB, MUL, AND, OR, XOR):
            ops.append((ld, insn(ALU | op | K, k=kk)))
            ops.append((insn(LDX | IMM, k=kk), ld, insn(ALU | op | X)))
    ops.append((ld, insn(ALU | NEG)))
    ops.append((insn(LD | IMM, k=0), insn(ALU | NEG)))  # NEG of 0
    ops.append((insn(LD | W | ABS, k=4), insn(MISC | TAX), ld, insn(ALU | MUL | X)))  # MUL overflow, both from bytes
    out.append(Case("alu_ops", d, o, c, [accumulate(ops)]))
    ops = []
    for kk in (1, 2, 3, 0x10000, 0x7FFFFFFF, 0x80000000, M32):
        for op in (DIV, MOD):
            ops.append((ld, insn(ALU | op | K, k=kk)))
            ops.append((insn(LDX | IMM, k=kk), ld, insn(ALU | op | X)))
    out.append(Case("alu_div_mod", d, o, c, [accumulate(ops)]))
    # DIV / MOD by X of 0 and 1: X = P[4] & 1, so about half of the packets are rejected there
    for op, nm in ((DIV, "div"), (MOD, "mod")):
        out.append(Case(f"alu_{nm}_x_0_1", d, o, c,
                        [prog(insn(LD | B | ABS, k=4), insn(ALU | AND | K, k=1), insn(MISC | TAX), ld,
                              insn(ALU | op | X), insn(ALU | ADD | K, k=1), insn(RET | A))]))
    out.append(Case("neg_zero_rejects", d, o, c, [prog(insn(LD | IMM, k=0), insn(ALU | NEG), insn(RET | A))]))
    # all 16 M[] slots through ST and STX, read back through LD and LDX; a slot never written reads 0
    rows = []
    for s in range(15):
        rows += [insn(LD | B | ABS, k=s % 12), insn(ALU | ADD | K, k=s * 257)]
        rows += [insn(ST, k=s)] if s % 2 else [insn(MISC | TAX), insn(STX, k=s)]
    rows += [insn(LD | MEM, k=15)]  # never written
    for s in range(15):
        rows += [insn(ALU | MUL | K, k=31)]
        rows += [insn(LDX | MEM, k=s), insn(ALU | ADD | X)] if s % 2 else \
            [insn(MISC | TAX), insn(LD | MEM, k=s), insn(ALU | ADD | X)]
    rows += [insn(ALU | OR | K, k=1), insn(RET | A)]
    out.append(Case("mem_all_slots", d, o, c, [bpf.program(rows)]))
    out.append(Case("mem_unwritten", d, o, c,
                    [prog(insn(LD | MEM, k=9), insn(LDX | MEM, k=15), insn(ALU | ADD | X), insn(ALU | ADD | K, k=5),
                          insn(RET | A))]))
    # LEN with and without frame_lens (a zero wire length returns 0)
    fl = np.random.default_rng(510).integers(0, 1 << 32, 70, dtype=np.uint64).astype(np.uint32)
    fl[:4] = (0, 1, M32, 12)
    p_len = prog(insn(LD | W | LEN), insn(RET | A))
    p_lenx = prog(insn(LDX | W | LEN), insn(MISC | TXA), insn(ALU | XOR | K, k=0x55), insn(RET | A))
    out.append(Case("len_caplen", d, o, c, [p_len]))
    out.append(Case("len_frame", d, o, c, [p_len], frame_lens=fl))
    out.append(Case("lenx_caplen", d, o, c, [p_lenx]))
    out.append(Case("lenx_frame", d, o, c, [p_lenx], frame_lens=fl))
    return out


def divergent_program() -> np.ndarray:
    """A jeq chain on P[0]: 64 branches, each its own ALU sequence over be32 P[1..4] ending in RET|A."""
    rows = [insn(LD | B | ABS, k=0), insn(MISC | TAX)]
    ops = (ADD, SUB, MUL, XOR, OR, AND, LSH, RSH)
    for v in range(64):
        rows.append(insn(MISC | TXA))  # A = P[0] again
        rows.append(insn(JMP | JEQ | K, 0, 4, v))
        rows += [insn(LD | W | ABS, k=1), insn(ALU | ops[v % 8] | K, k=(v * 0x9E3779B1 + 3) & (31 if v % 8 >= 6 else M32)),
                 insn(ALU | ops[(v // 8) % 6] | K, k=v + 1), insn(RET | A)]
    rows.append(insn(RET | K, k=0))
    return bpf.program(rows)


def long_program() -> np.ndarray:
    """4096 instructions, accepting only at the last one; every third one a conditional skip of the next."""
    n = abi.BPF_MAX_INSNS
    rows = [insn(LD | W | ABS, k=0)]
    for i in range(1, n - 1):
        if i % 3 == 0 and i < n - 3:
            rows.append(insn(JMP | JSET | K, 1, 0, 1 << (i % 7)))
        elif i % 3 == 1:
            rows.append(insn(ALU | ADD | K, k=i * 2654435761 & M32))
        else:
            rows.append(insn(ALU | XOR | K, k=i * 40503 & M32))
    rows.append(insn(RET | A))
    assert len(rows) == n
    return bpf.program(rows)


def control_cases() -> list[Case]:
    out = []
    d, o, c = packed(np.full(129, 9, np.uint32), 600)
    d[0::9][:129] = np.arange(129) % 67  # P[0] differs per lane; 64, 65, 66 take no branch
    out.append(Case("divergent_64", d, o, c, [divergent_program()]))
    d2, o2, c2 = packed(np.full(65, 8, np.uint32), 601)
    out.append(Case("long_4096", d2, o2, c2, [long_program()]))
    # JA with a large k over instructions that would return something else
    n = 3000
    rows = [insn(LD | B | ABS, k=0), insn(JMP | JA, k=n - 3)] + [insn(RET | K, k=9)] * (n - 3) + [insn(RET | A)]
    out.append(Case("ja_far", d2, o2, c2, [bpf.program(rows)]))
    out.append(Case("ja_zero", d2, o2, c2, [prog(insn(JMP | JA, k=0), insn(LD | B | ABS, k=1), insn(RET | A))]))
    # jt / jf of 255
    for nm, jt, jf in (("jt255", 255, 0), ("jf255", 0, 255)):
        rows = [insn(LD | B | ABS, k=0), insn(JMP | JSET | K, jt, jf, 1), insn(RET | K, k=1)] + \
               [insn(RET | K, k=2)] * 254 + [insn(RET | K, k=3)]
        out.append(Case(nm, d2, o2, c2, [bpf.program(rows)]))
    # every comparison through K and X around equality
    for op, nm in ((JEQ, "jeq"), (JGT, "jgt"), (JGE, "jge"), (JSET, "jset")):
        out.append(Case(f"{nm}_k", d, o, c, [prog(insn(LD | B | ABS, k=0), insn(JMP | op | K, 0, 1, 33),
                                                   insn(RET | K, k=5), insn(RET | K, k=0))]))
        out.append(Case(f"{nm}_x", d, o, c, [prog(insn(LD | B | ABS, k=1), insn(ALU | AND | K, k=63), insn(MISC | TAX),
                                                   insn(LD | B | ABS, k=0), insn(JMP | op | X, 0, 1, 0),
                                                   insn(RET | K, k=5), insn(RET | K, k=M32))]))
    out.append(Case("jgt_unsigned", d, o, c, [prog(insn(LD | W | ABS, k=1), insn(JMP | JGT | K, 0, 1, 0x7FFFFFFF),
                                                    insn(RET | K, k=1), insn(RET | K, k=2))]))
    out.append(Case("ret0", d, o, c, [prog(insn(RET | K, k=0))]))
    out.append(Case("ret7", d, o, c, [prog(insn(RET | K, k=7))]))
    out.append(Case("ret_max", d, o, c, [prog(insn(RET | K, k=M32))]))
    return out


def classifier(q: int) -> np.ndarray:
    """Program q of a set: accepts when (P[0] & 15) == q or P[1] > 200 + 3 * q, and returns 100 + q plus M[q - 1], a
    slot the program before it wrote on the same lane: every program starts with M[] zero."""
    return prog(insn(LD | IMM, k=0xDEAD00 + q), insn(ST, k=q), insn(LD | B | ABS, k=0), insn(ALU | AND | K, k=15),
                insn(JMP | JEQ | K, 2, 0, q), insn(LD | B | ABS, k=1), insn(JMP | JGT | K, 0, 3, 200 + 3 * q),
                insn(LD | MEM, k=(q + 15) % 16), insn(ALU | ADD | K, k=100 + q), insn(RET | A), insn(RET | K, k=0))


def multi_cases() -> list[Case]:
    out = []
    d, o, c = packed(np.concatenate([np.full(300, 6, np.uint32), [1, 0, 2]]).astype(np.uint32), 700)
    for P in (2, 3, 16):
        out.append(Case(f"programs_{P}", d, o, c, [classifier(q) for q in range(P)]))
    out.append(Case("first_rejects_all", d, o, c, [prog(insn(RET | K, k=0)), classifier(1), classifier(0)]))
    out.append(Case("all_reject", d, o, c, [prog(insn(RET | K, k=0))] * 16))
    out.append(Case("first_accepts_all", d, o, c, [prog(insn(RET | K, k=1)), classifier(1)]))
    # NULL columns: the buffers are not passed and keep their fill
    base = out[2]
    for cols in (("matched",), ("bucket",), ("ret",), (), ("matched", "ret")):
        out.append(Case("columns_" + ("_".join(cols) or "none"), d, o, c, base.programs, columns=cols))
    return out


# ---------------------------------------------------------------- more chunks than the grid has blocks
CHUNK, MAX_BLOCKS = 256, 8192  # pcppx_bpf.hip: packets per block and step, and the grid's size limit
P_ODD = prog(insn(LD | B | ABS, k=0), insn(JMP | JSET | K, 0, 2, 1), insn(LD | B | ABS, k=1), insn(RET | A),
             insn(RET | K, k=0))


@lru_cache(maxsize=None)
def grid_stride():
    """(case, expected Result): 2-byte packets, a quarter more chunks (and a partial one) than the grid has blocks, so
    the first quarter of the blocks walk two chunks and the others one; a bad descriptor every 1000 packets.
    The program accepts when P[0] is odd and returns P[1]: the expected columns come from numpy (the interpreter is a
    Python loop), and the C++ reference is compared with them on the CPU."""
    n = CHUNK * (MAX_BLOCKS + MAX_BLOCKS // 4) + 77
    d, o, c = packed(np.full(n, 2, np.uint32), 900)
    o = o.copy()
    o[::1000] = len(d) - 1  # one byte past the end
    case = Case("grid_stride", d, o, c, [P_ODD])
    want = blank(n)
    idx = o.astype(np.int64)
    live = idx + 2 <= len(d)
    b0 = d[np.minimum(idx, len(d) - 2)]
    b1 = d[np.minimum(idx, len(d) - 2) + 1]
    m = live & ((b0 & 1) != 0) & (b1 != 0)
    want.matched[:n] = m
    want.bucket[:n] = np.where(m, 0, 0xFF)
    want.ret[:n] = np.where(m, b1, 0)
    want.totals[:] = 0
    want.totals[abi.BPF_MATCHED] = int(m.sum())
    want.totals[abi.BPF_BAD_DESC] = int((~live).sum())
    return case, want


# ---------------------------------------------------------------- fuzz
FUZZ_PROGRAMS, FUZZ_PACKETS = 200, 256


def fuzz_program(rng: np.random.Generator) -> np.ndarray:
    """A valid random program: every opcode, forward jumps, the returns in the last two places."""
    n = int(rng.integers(6, 40))
    body = n - 2
    rows = []
    small = lambda: int(rng.integers(0, 48))  # noqa: E731
    word = lambda: int(rng.choice([0, 1, 2, 0xFF, 0xFFFF, 0x80000000, M32, int(rng.integers(0, 1 << 32))]))  # noqa: E731
    for i in range(body):
        left = body - 1 - i  # body instructions behind this one
        kind = rng.choice(["ld", "ldx", "st", "alu", "jmp", "misc"], p=[0.30, 0.12, 0.08, 0.25, 0.17, 0.08])
        if kind == "ld":
            mode = rng.choice(["abs", "ind", "imm", "mem", "len"], p=[0.45, 0.25, 0.1, 0.1, 0.1])
            sz = int(rng.choice([W, H, B]))
            if mode == "abs":
                rows.append(insn(LD | sz | ABS, k=small()))
            elif mode == "ind":
                rows.append(insn(LD | sz | IND, k=int(rng.integers(0, 24))))
            elif mode == "imm":
                rows.append(insn(LD | IMM, k=word()))
            elif mode == "mem":
                rows.append(insn(LD | MEM, k=int(rng.integers(0, 16))))
            else:
                rows.append(insn(LD | W | LEN))
        elif kind == "ldx":
            mode = rng.choice(["imm", "msh", "mem", "len"], p=[0.4, 0.4, 0.1, 0.1])
            rows.append({"imm": insn(LDX | IMM, k=int(rng.integers(0, 40))), "msh": insn(LDX | B | MSH, k=small()),
                         "mem": insn(LDX | MEM, k=int(rng.integers(0, 16))), "len": insn(LDX | W | LEN)}[mode])
        elif kind == "st":
            rows.append(insn(int(rng.choice([ST, STX])), k=int(rng.integers(0, 16))))
        elif kind == "alu":
            op = int(rng.choice([ADD, SUB, MUL, DIV, MOD, AND, OR, XOR, LSH, RSH, NEG]))
            if op == NEG:
                rows.append(insn(ALU | NEG))
            elif rng.random() < 0.3:
                rows.append(insn(ALU | op | X))
            else:
                k = int(rng.integers(0, 36)) if op in (LSH, RSH) else word()
                rows.append(insn(ALU | op | K, k=max(k, 1) if op in (DIV, MOD) else k))
        elif kind == "jmp":
            if rng.random() < 0.15:
                rows.append(insn(JMP | JA, k=int(rng.integers(0, min(left, 3) + 1))))
            else:
                op = int(rng.choice([JEQ, JGT, JGE, JSET]))
                far = min(left + 1, 4)  # up to the first return
                src = X if rng.random() < 0.3 else K
                rows.append(insn(JMP | op | src, int(rng.integers(0, far + 1)), int(rng.integers(0, far + 1)),
                                 int(rng.choice([0, 1, 0x80, 0x800, 6, 17, int(rng.integers(0, 256))]))))
        else:
            rows.append(insn(MISC | int(rng.choice([TAX, TXA]))))
    # the two returns: a value of A that is zero rejects; one of the two constants is usually zero
    first = insn(RET | K, k=0) if rng.random() < 0.6 else insn(RET | A)
    last = insn(RET | K, k=int(rng.integers(1, 1 << 18))) if rng.random() < 0.6 else insn(RET | A)
    rows += [first, last]
    return bpf.program(rows)


@lru_cache(maxsize=None)
def fuzz():
    """(the packet batch as a Case without programs, the programs, the interpreter's Result per program, the sums of
    the interpreter's statistics). Computed once."""
    rng = np.random.default_rng(20240611)
    lens = rng.integers(30, 120, FUZZ_PACKETS).astype(np.uint32)
    lens[:4] = (0, 1, 60, 119)
    d, o, c = packed(lens, 800, lead=3)
    fl = (lens + rng.integers(0, 3, FUZZ_PACKETS) * 100).astype(np.uint32)
    programs = [fuzz_program(rng) for _ in range(FUZZ_PROGRAMS)]
    results, stats = [], {"pairs": 0, "accepted": 0, "oob": 0, "steps4": 0}
    for j, p in enumerate(programs):
        r = interp(fuzz_case(d, o, c, fl, p, j))
        results.append(r)
        for k in stats:
            stats[k] += r.stats[k]
    return (d, o, c, fl), programs, results, stats


def fuzz_case(d, o, c, fl, p, j) -> Case:
    return Case(f"fuzz{j}", d, o, c, [p], frame_lens=fl, misalign=3)


@lru_cache(maxsize=None)
def cases() -> tuple:
    out = shape_cases() + load_edge_cases() + alu_cases() + control_cases() + multi_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    for c in out:
        for p in c.programs:
            assert abi.bpf_validate(p), c.name
    return tuple(out)


@lru_cache(maxsize=None)
def expected(name: str) -> Result:
    """The interpreter's result for a case: computed once, shared by the CPU and the GPU tests, never modified."""
    return interp({c.name: c for c in cases()}[name])


# ---------------------------------------------------------------- the hand-written real filter
def tcp_dst_port_program(port: int) -> np.ndarray:
    return bpf.tcp_dst_port(port)


def as_case(name: str, batch, programs, frame_lens=None) -> Case:
    return Case(name, np.ascontiguousarray(batch.data), np.ascontiguousarray(batch.offsets, dtype=np.uint64),
                np.ascontiguousarray(batch.caplens, dtype=np.uint32), programs, frame_lens=frame_lens)
