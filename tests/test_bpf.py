"""pcppx_bpf_device: classic BPF filter programs run over the packets of a device batch (include/pcppx.h, bpf).

CPU: pcppx_bpf_reference (the contract in plain C++ over host pointers) equals the per-packet Python interpreter of
tests/bpf_cases.py on every case family and on the fuzz, whose generator meets its coverage conditions on the
interpreter alone; the ctypes mirrors match the header; every validator rule refuses its offending program and accepts
the nearest legal one; every bad-argument combination is refused without a GPU; parse_dd round-trips both tcpdump
forms; a hand-written "tcp dst port" filter agrees with the predicate computed from the restatement's 5-tuples.
GPU: pcppx_bpf_device equals pcppx_bpf_reference byte for byte -- matched, bucket, ret, totals, and the 0xA5 fill past n
and of columns left NULL -- on the same cases and the fuzz; the real filter agrees with the tuples of a device parse;
matched feeds pcppx_select_device and bucket feeds pcppx_steer_device on the device; two calls on two streams agree;
packets on both sides of offset 2^32 of one allocation are filtered exactly.
"""
from __future__ import annotations

import ctypes as C
import re
import subprocess
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import bpf_cases as bc
import oracle
import select_cases as sc
import steer_cases as tc
import wide_cases as wc
from conftest import GOLDEN, load_golden
from pcapplusplus_amd import abi, bpf, synth
from pcapplusplus_amd.bpf import ABS, ALU, DIV, IMM, JA, JEQ, JMP, LD, LDX, MEM, MOD, RET, ST, STX, A, B, H, K, W, X, insn

HEADER = abi.REPO_DIR / "include" / "pcppx.h"
DEV = "cuda:0"
CASES = bc.cases()
BY_NAME = {c.name: c for c in CASES}
PORT = 443


# ---------------------------------------------------------------- CPU: the reference against the interpreter
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_reference_equals_interpreter(case):
    bc.assert_same(bc.run_reference(case), bc.expected(case.name), case.name)


def test_cases_reach_what_they_name():
    exp = {c.name: bc.expected(c.name) for c in CASES}
    assert {c.n for c in CASES} >= {0, 1, 63, 64, 65, 129, 1000}
    assert {c.misalign for c in CASES} >= set(range(8))
    caps = BY_NAME["caplens_0_1_3_4_70000"]
    assert set(caps.caplens.tolist()) >= {0, 1, 3, 4, 70000}
    assert int(caps.offsets[-1]) + int(caps.caplens[-1]) == caps.dlen()
    big = np.nonzero(caps.caplens == 70000)[0]
    assert exp[caps.name].matched[big].all()  # read at their first and last byte, above PCPPX_MAX_CAPLEN
    bad = exp["bad_desc"]
    assert int(bad.totals[abi.BPF_BAD_DESC]) == 6
    for i in (3, 64, 65, 70, 71, 129):
        assert (bad.matched[i], bad.bucket[i], bad.ret[i]) == (0, 0xFF, 0)
    assert bad.matched[100] == 1  # ends exactly at data_len
    # the load edges: with k fixed, the caplens on both sides of every bound accept / reject
    k = 21
    for nm, size in (("w", 4), ("h", 2), ("b", 1)):
        c = BY_NAME[f"abs_{nm}"]
        fits = c.caplens >= k + size
        for name in (f"abs_{nm}", f"ind_{nm}_x0", f"ind_{nm}_x21", f"ind_{nm}_x7"):
            assert np.array_equal(exp[name].matched[:c.n] != 0, fits), name
        assert {k + size - 1, k + size, k + size + 1, k - 1, k} <= set(c.caplens.tolist())
        assert np.array_equal(exp[f"ind_{nm}_last"].matched[:c.n] != 0, c.caplens >= size)
        for name in (f"ind_{nm}_x_caplen", f"ind_{nm}_wrap", f"ind_{nm}_kmax", f"ind_{nm}_kmax_x2", f"abs_{nm}_kmax"):
            assert not exp[name].matched[:c.n].any(), name
    c = BY_NAME["msh"]
    assert np.array_equal(exp["msh"].matched[:c.n] != 0, c.caplens >= k + 1)
    for name in ("alu_div_x_0_1", "alu_mod_x_0_1"):
        m = exp[name].matched[:BY_NAME[name].n]
        assert 10 < int(m.sum()) < len(m) - 10, name  # X == 0 rejects, X == 1 goes on
    assert not exp["neg_zero_rejects"].matched[:70].any()
    assert exp["mem_unwritten"].ret[:70].tolist() == [5] * 70
    fl = BY_NAME["len_frame"].frame_lens
    assert np.array_equal(exp["len_frame"].ret[:70], fl) and exp["len_caplen"].ret[:70].tolist() == [12] * 70
    d = BY_NAME["divergent_64"]
    first = d.data[d.offsets[:64].astype(np.int64)]
    assert sorted(first.tolist()) == list(range(64))  # every lane of the first tile takes another branch
    assert len(BY_NAME["long_4096"].programs[0]) == abi.BPF_MAX_INSNS
    assert set(np.unique(BY_NAME["long_4096"].programs[0]["code"][:-1]).tolist()).isdisjoint({RET | K, RET | A})
    far = BY_NAME["ja_far"]
    assert np.array_equal(exp["ja_far"].ret[:far.n], far.data[far.offsets.astype(np.int64)])  # never the 9 it jumps over
    assert set(exp["jt255"].ret[:65].tolist()) == {1, 3} and set(exp["jf255"].ret[:65].tolist()) == {1, 3}
    for P in (2, 3, 16):
        r = exp[f"programs_{P}"]
        n = BY_NAME[f"programs_{P}"].n
        assert set(r.bucket[:n].tolist()) >= set(range(P))
        assert np.array_equal(r.ret[:n][r.matched[:n] != 0], 100 + r.bucket[:n][r.matched[:n] != 0])  # M[] starts at zero
    assert (exp["programs_3"].bucket[:303] == 0xFF).sum() > 100  # accepted by none
    r16 = exp["programs_16"]
    c16 = BY_NAME["programs_16"]
    several = sum(1 for i in range(300) if c16.data[int(c16.offsets[i]) + 1] > 245 and r16.bucket[i] == 0)
    assert several > 3  # accepted by every program: the lowest index wins
    r = exp["first_rejects_all"]
    assert set(r.bucket[:303].tolist()) == {1, 2, 0xFF}


def test_grid_stride_case_passes_the_grid_and_the_reference_equals_numpy():
    """The one case above 1000 packets: the batch has more 256-packet chunks than the kernel's grid has blocks, the
    path on which a block takes several chunks. Its size follows the kernel's constants."""
    txt = (abi.PKG_DIR / "csrc" / "pcppx_bpf.hip").read_text()
    assert int(re.search(r"kBpfMaxBlocks\s*=\s*(\d+)", txt).group(1)) == bc.MAX_BLOCKS
    assert int(re.search(r"kBpfThreads\s*=\s*(\d+)", txt).group(1)) == bc.CHUNK
    case, want = bc.grid_stride()
    chunks = -(-case.n // bc.CHUNK)
    assert bc.MAX_BLOCKS + 1000 < chunks < 2 * bc.MAX_BLOCKS and case.n % bc.CHUNK != 0
    assert int(want.totals[abi.BPF_BAD_DESC]) > 1000 and 0.3 * case.n < int(want.totals[abi.BPF_MATCHED]) < 0.7 * case.n
    bc.assert_same(bc.run_reference(case), want, case.name)
    head = replace(case, name="grid_stride_head", offsets=case.offsets[:3000].copy(), caplens=case.caplens[:3000].copy())
    got = bc.interp(head)  # the numpy expectation against the interpreter, on the first packets
    assert np.array_equal(got.matched[:3000], want.matched[:3000]) and np.array_equal(got.ret[:3000], want.ret[:3000])
    assert np.array_equal(got.bucket[:3000], want.bucket[:3000])


def test_fuzz_meets_its_conditions():
    """On the Python interpreter alone: the generator is tuned, the bounds are the issue's."""
    _, programs, _, st = bc.fuzz()
    assert len(programs) == 200 and st["pairs"] == 200 * 256
    print("fuzz:", {k: round(v / st["pairs"], 4) for k, v in st.items()})
    assert 0.20 <= st["accepted"] / st["pairs"] <= 0.80
    assert st["oob"] / st["pairs"] >= 0.05
    assert st["steps4"] / st["pairs"] >= 0.50
    codes = set(np.concatenate([p["code"] for p in programs]).tolist())
    every = {LD | s | m for s in (W, H, B) for m in (ABS, bpf.IND)} | \
        {LD | IMM, LD | MEM, LD | W | bpf.LEN, LDX | IMM, LDX | MEM, LDX | W | bpf.LEN, LDX | B | bpf.MSH, ST, STX,
         ALU | bpf.NEG, JMP | JA, RET | K, RET | A, bpf.MISC | bpf.TAX, bpf.MISC | bpf.TXA} | \
        {ALU | op | s for op in (bpf.ADD, bpf.SUB, bpf.MUL, DIV, MOD, bpf.AND, bpf.OR, bpf.XOR, bpf.LSH, bpf.RSH)
         for s in (K, X)} | {JMP | op | s for op in (JEQ, bpf.JGT, bpf.JGE, bpf.JSET) for s in (K, X)}
    assert every <= codes, sorted(every - codes)
    for p in programs:
        assert abi.bpf_validate(p)


def test_reference_equals_interpreter_on_the_fuzz():
    (d, o, c, fl), programs, results, _ = bc.fuzz()
    for j, (p, want) in enumerate(zip(programs, results)):
        bc.assert_same(bc.run_reference(bc.fuzz_case(d, o, c, fl, p, j)), want, f"fuzz{j}")


# ---------------------------------------------------------------- CPU: mirrors, validator, bad arguments, parse_dd
def test_bpf_structs_match_header():
    fields = {"pcppx_bpf_insn": abi.BpfInsn, "pcppx_bpf_prog": abi.BpfProg, "pcppx_bpf_verdicts": abi.BpfVerdicts}
    lines = "".join(f'  printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));\n'
                    for t, cls in fields.items() for f, _ in cls._fields_)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pcppx.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu\\n", sizeof(pcppx_bpf_insn), sizeof(pcppx_bpf_prog), sizeof(pcppx_bpf_verdicts));\n'
           '  printf("%d %d %d %d %d %d %d\\n", PCPPX_BPF_MAX_INSNS, PCPPX_BPF_MAX_PROGRAMS, PCPPX_BPF_MEMWORDS,\n'
           '         PCPPX_BPF_MATCHED, PCPPX_BPF_BAD_DESC, PCPPX_BPF_TOTALS, PCPPX_ABI_VERSION);\n' + lines +
           "  return 0; }\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "b.c"
        c.write_text(src)
        exe = Path(d) / "b"
        subprocess.run(["gcc", "-I", str(HEADER.parent), str(c), "-o", str(exe)], check=True)
        out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert [int(x) for x in out[0].split()] == [C.sizeof(abi.BpfInsn), C.sizeof(abi.BpfProg), C.sizeof(abi.BpfVerdicts)]
    assert [int(x) for x in out[1].split()] == [abi.BPF_MAX_INSNS, abi.BPF_MAX_PROGRAMS, abi.BPF_MEMWORDS,
                                                abi.BPF_MATCHED, abi.BPF_BAD_DESC, abi.BPF_TOTALS, abi.ABI_VERSION]
    seen = 0
    for line in out[2:]:
        name, off, size = line.split()
        t, f = name.split(".")
        d = getattr(fields[t], f)
        assert (d.offset, d.size) == (int(off), int(size)), name
        seen += 1
    assert seen == sum(len(cls._fields_) for cls in fields.values())
    assert abi.ABI_VERSION == 7 and abi.BPF_INSN_DTYPE.itemsize == C.sizeof(abi.BpfInsn) == 8
    for f, _ in abi.BpfInsn._fields_:
        assert abi.BPF_INSN_DTYPE.fields[f][1] == getattr(abi.BpfInsn, f).offset


RET1 = insn(RET | K, k=1)
NOP = insn(LD | IMM, k=0)
# rule -> (a program the validator refuses, its nearest legal neighbour)
VALIDATOR = {
    "jt_at_n": ([insn(JMP | JEQ | K, 2, 0, 0), RET1, RET1], [insn(JMP | JEQ | K, 1, 0, 0), RET1, RET1]),
    "jf_at_n": ([insn(JMP | JEQ | K, 0, 2, 0), RET1, RET1], [insn(JMP | JEQ | K, 0, 1, 0), RET1, RET1]),
    "jt_255_short": ([insn(JMP | JEQ | X, 255, 0, 0)] + [RET1] * 255, [insn(JMP | JEQ | X, 255, 0, 0)] + [RET1] * 256),
    "ja_at_n": ([insn(JMP | JA, k=2), RET1, RET1], [insn(JMP | JA, k=1), RET1, RET1]),
    "ja_wraps": ([NOP, insn(JMP | JA, k=0xFFFFFFFF), RET1], [NOP, insn(JMP | JA, k=0), RET1]),
    "ja_wraps_to_next": ([NOP, insn(JMP | JA, k=0xFFFFFFFE), RET1, RET1], [NOP, insn(JMP | JA, k=1), RET1, RET1]),
    "ld_mem_16": ([insn(LD | MEM, k=16), RET1], [insn(LD | MEM, k=15), RET1]),
    "ldx_mem_16": ([insn(LDX | MEM, k=16), RET1], [insn(LDX | MEM, k=15), RET1]),
    "st_16": ([insn(ST, k=16), RET1], [insn(ST, k=15), RET1]),
    "stx_16": ([insn(STX, k=16), RET1], [insn(STX, k=15), RET1]),
    "st_huge": ([insn(ST, k=0x80000000), RET1], [insn(ST, k=0), RET1]),
    "div_k0": ([insn(ALU | DIV | K, k=0), RET1], [insn(ALU | DIV | K, k=1), RET1]),
    "mod_k0": ([insn(ALU | MOD | K, k=0), RET1], [insn(ALU | MOD | K, k=1), RET1]),
    "div_x_k0_is_legal": ([insn(ALU | DIV | K, k=0), RET1], [insn(ALU | DIV | X, k=0), RET1]),
    "no_final_ret": ([RET1, NOP], [NOP, RET1]),
    "ends_in_jump": ([RET1, insn(JMP | JA, k=0)], [insn(JMP | JA, k=0), RET1]),
    "ret_x": ([insn(RET | X)], [insn(RET | A)]),
    "unknown_class_bits": ([insn(0x0100 | RET | K, k=1)], [RET1]),
    "ld_w_msh": ([insn(LD | W | bpf.MSH, k=0), RET1], [insn(LDX | B | bpf.MSH, k=0), RET1]),
    "ldx_abs": ([insn(LDX | W | ABS, k=0), RET1], [insn(LD | W | ABS, k=0), RET1]),
    "ld_size_3": ([insn(LD | 0x18 | ABS, k=0), RET1], [insn(LD | B | ABS, k=0), RET1]),
    "alu_op_b0": ([insn(ALU | 0xB0, k=1), RET1], [insn(ALU | bpf.XOR, k=1), RET1]),
    "neg_x": ([insn(ALU | bpf.NEG | X), RET1], [insn(ALU | bpf.NEG), RET1]),
    "jmp_op_50": ([insn(JMP | 0x50, 0, 0, 0), RET1], [insn(JMP | bpf.JSET, 0, 0, 0), RET1]),
    "ja_x": ([insn(JMP | JA | X, k=0), RET1], [insn(JMP | JA, k=0), RET1]),
    "misc_other": ([insn(bpf.MISC | 0x40), RET1], [insn(bpf.MISC | bpf.TXA), RET1]),
}


@pytest.mark.parametrize("rule", sorted(VALIDATOR))
def test_validator_refuses_and_accepts(rule):
    bad, good = VALIDATOR[rule]
    assert not abi.bpf_validate(bad), rule
    assert abi.bpf_validate(good), rule
    # pcppx_bpf_reference applies the same rules per program
    d, o, c = bc.packed([8, 8], 1)
    case = bc.Case(rule, d, o, c, [bpf.program(good)])
    bc.run_reference(case)
    with pytest.raises(RuntimeError):
        bc.run_reference(replace(case, programs=[bpf.program(good), bpf.program(bad)]))


def test_validator_program_length():
    lib = abi.load_engine()
    body = [NOP] * (abi.BPF_MAX_INSNS - 1)
    assert abi.bpf_validate(body + [RET1])                 # 4096
    assert not abi.bpf_validate(body + [NOP, RET1])        # 4097
    assert abi.bpf_validate([RET1])
    one = bpf.program([RET1])
    assert lib.pcppx_bpf_validate(one.ctypes.data, 0) == abi.E_INVAL   # no instructions
    assert lib.pcppx_bpf_validate(None, 1) == abi.E_INVAL


def _good_reference_args():
    d, o, c = bc.packed([8, 8], 1)
    progs, keep = abi.make_bpf_progs([bpf.program([RET1])])
    b = abi.Batch(d.ctypes.data, o.ctypes.data, c.ctypes.data, len(d), 2, 1, 0)
    res = bc.blank(2)
    return progs, b, bc.verdicts(res, bc.COLUMNS), (d, o, c, keep, res)


def test_bad_arguments_return_einval_without_gpu():
    lib = abi.load_engine()
    progs, b, v, alive = _good_reference_args()
    ref = lambda p, n, bb, vv: lib.pcppx_bpf_reference(p, n, bb, None, vv)  # noqa: E731
    assert ref(progs, 1, C.byref(b), C.byref(v)) == abi.OK
    assert ref(None, 1, C.byref(b), C.byref(v)) == abi.E_INVAL
    assert ref(progs, 0, C.byref(b), C.byref(v)) == abi.E_INVAL
    assert ref(progs, 1, None, C.byref(v)) == abi.E_INVAL
    assert ref(progs, 1, C.byref(b), None) == abi.E_INVAL
    many = (abi.BpfProg * 17)(*([progs[0]] * 17))
    assert ref(many, 16, C.byref(b), C.byref(v)) == abi.OK
    assert ref(many, 17, C.byref(b), C.byref(v)) == abi.E_INVAL
    no_totals = abi.BpfVerdicts(v.matched, v.bucket, v.ret, None)
    assert ref(progs, 1, C.byref(b), C.byref(no_totals)) == abi.E_INVAL
    null_insns = (abi.BpfProg * 1)(abi.BpfProg(None, 1, 0))
    assert ref(null_insns, 1, C.byref(b), C.byref(v)) == abi.E_INVAL
    reserved = (abi.BpfProg * 1)(abi.BpfProg(progs[0].insns, 1, 1))
    assert ref(reserved, 1, C.byref(b), C.byref(v)) == abi.E_INVAL
    empty = (abi.BpfProg * 1)(abi.BpfProg(progs[0].insns, 0, 0))
    assert ref(empty, 1, C.byref(b), C.byref(v)) == abi.E_INVAL
    no_offsets = abi.Batch(b.data, None, b.caplens, b.data_len, 2, 1, 0)
    assert ref(progs, 1, C.byref(no_offsets), C.byref(v)) == abi.E_INVAL
    # the device entry points: the argument checks come before any device work (the handles are never dereferenced)
    ctx, f, out = C.c_void_p(1), C.c_void_p(1), C.c_void_p()
    dev = lambda cc, ff, bb, vv: lib.pcppx_bpf_device(cc, ff, bb, None, vv, None)  # noqa: E731
    assert dev(None, f, C.byref(b), C.byref(v)) == abi.E_INVAL
    assert dev(ctx, None, C.byref(b), C.byref(v)) == abi.E_INVAL
    assert dev(ctx, f, None, C.byref(v)) == abi.E_INVAL
    assert dev(ctx, f, C.byref(b), None) == abi.E_INVAL
    assert dev(ctx, f, C.byref(b), C.byref(no_totals)) == abi.E_INVAL
    assert dev(ctx, f, C.byref(no_offsets), C.byref(v)) == abi.E_INVAL
    load = lambda cc, p, n, o: lib.pcppx_bpf_load(cc, p, n, o)  # noqa: E731
    assert load(None, progs, 1, C.byref(out)) == abi.E_INVAL
    assert load(ctx, None, 1, C.byref(out)) == abi.E_INVAL
    assert load(ctx, progs, 0, C.byref(out)) == abi.E_INVAL
    assert load(ctx, many, 17, C.byref(out)) == abi.E_INVAL
    assert load(ctx, progs, 1, None) == abi.E_INVAL
    assert load(ctx, null_insns, 1, C.byref(out)) == abi.E_INVAL
    assert load(ctx, reserved, 1, C.byref(out)) == abi.E_INVAL
    assert load(ctx, empty, 1, C.byref(out)) == abi.E_INVAL
    bad_prog, _keep = abi.make_bpf_progs([bpf.program([NOP])])
    assert load(ctx, bad_prog, 1, C.byref(out)) == abi.E_INVAL
    assert not out.value
    lib.pcppx_bpf_free(None)  # a no-op
    del alive


def test_n0_is_legal_and_writes_zero_totals():
    got = bc.run_reference(BY_NAME["n0"])
    assert got.totals.tolist() == [0] * abi.BPF_TOTALS
    assert (got.matched == bc.FILL).all() and (got.bucket == bc.FILL).all()


def test_parse_dd_round_trips_both_forms():
    p = bpf.tcp_dst_port(PORT)
    dd, ddd = bpf.format_dd(p), bpf.format_ddd(p)
    assert dd.splitlines()[0] == "{ 0x28, 0, 0, 0x0000000c }," and ddd.splitlines()[:2] == ["11", "40 0 0 12"]
    for text in (dd, ddd, dd.replace("\n", " "), "\n" + ddd + "\n"):
        q = bpf.parse_dd(text)
        assert q.dtype == bpf.INSN_DTYPE and np.array_equal(q, p)
    big = bc.long_program()
    assert np.array_equal(bpf.parse_dd(bpf.format_dd(big)), big)
    assert np.array_equal(bpf.parse_dd(bpf.format_ddd(big)), big)
    for junk in ("", "3\n6 0 0 1\n", "{ 0x6, 0, 0, 0x1 }, oops", "1\n6 0 0\n", "{ 0x6, 0, 0, 0x100000000 },"):
        with pytest.raises(ValueError):
            bpf.parse_dd(junk)
    assert bpf.insn(RET | K, k=5) == (6, 0, 0, 5)
    with pytest.raises(ValueError):
        bpf.insn(RET, jt=256)


# ---------------------------------------------------------------- the real filter against the parse
IPV4, TCP_PROTO = 2, 4  # pcpp::IPv4, pcpp::TCP (ProtocolType.h)


@pytest.fixture(scope="module")
def real_batches():
    """The plain-Ethernet synthetic batch with a tenth of its TCP destination ports set to PORT (the TCP checksum is
    not the filter's business), and the bundled example capture."""
    b = synth.small64(4000, 2)
    rng = np.random.default_rng(9)
    data = b.data.copy()
    for i in np.nonzero(rng.random(b.n) < 0.2)[0]:
        o = int(b.offsets[i])
        if data[o + 23] == 6:
            data[o + 36], data[o + 37] = PORT >> 8, PORT & 0xFF
    b = replace(b, data=data)
    ex, _ = load_golden(GOLDEN / "capture_example.npz")
    return {"synth": b, "example": ex}


def coincide(batch, tuples, layers) -> np.ndarray:
    """The packets on which "IPv4, not a later fragment, TCP, dst port P over untagged Ethernet" and the parse's
    (ip_version 4, l4_proto TCP, dst_port P) are the same statement: the chain is Ethernet, then directly IPv4 that is
    no fragment and directly TCP or no TCP at all (no VLAN tag, no tunnel), or it has no IPv4 layer at all."""
    n = batch.n
    ok = np.zeros(n, bool)
    for i in range(n):
        lay, t = layers[i], tuples[i]
        if t["flags"] & (abi.F_OVERSIZE | abi.F_BAD_DESC):
            continue
        if t["ip_version"] != 4:
            ok[i] = lay[0]["proto"] == 1 and (t["n_layers"] < 2 or lay[1]["proto"] != IPV4)
            continue
        if not (lay[0]["proto"] == 1 and lay[1]["proto"] == IPV4 and lay[1]["offset"] == 14):
            continue
        o = int(batch.offsets[i])
        frag = (int(batch.data[o + 20]) << 8 | int(batch.data[o + 21])) & 0x3FFF
        ok[i] = frag == 0 and (t["l4_proto"] != TCP_PROTO or (t["n_layers"] >= 3 and lay[2]["proto"] == TCP_PROTO))
    return ok


def predicate(tuples, port: int) -> np.ndarray:
    return (tuples["ip_version"] == 4) & (tuples["l4_proto"] == TCP_PROTO) & (tuples["dst_port"] == port)


def example_port(tuples) -> int:
    """The most frequent TCP destination port of a capture."""
    p = tuples["dst_port"][(tuples["ip_version"] == 4) & (tuples["l4_proto"] == TCP_PROTO)]
    vals, cnt = np.unique(p, return_counts=True)
    return int(vals[np.argmax(cnt)])


@pytest.mark.parametrize("which", ["synth", "example"])
def test_real_filter_equals_the_restatement_predicate(real_batches, which):
    b = real_batches[which]
    _, lay, tup = oracle.oracle_parse_tuples(b, abi.make_opts(0, 8, False, 8))
    port = PORT if which == "synth" else example_port(tup)
    keep = coincide(b, tup, lay)
    print(which, "coincide", int(keep.sum()), "of", b.n, "port", port)
    assert keep.sum() > 0.9 * b.n
    got = bc.run_reference(bc.as_case(which, b, [bpf.tcp_dst_port(port)]))
    want = predicate(tup, port)
    assert want[keep].sum() > 5
    assert np.array_equal(got.matched[:b.n][keep] != 0, want[keep])
    assert set(got.ret[:b.n][got.matched[:b.n] != 0].tolist()) == {262144}


# ---------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gpu_device_equals_reference(engine, case):
    want = bc.run_reference(case)
    bc.assert_same(want, bc.expected(case.name), case.name)
    bc.assert_same(bc.run_device(engine, case, DEV), want, case.name)


@pytest.mark.gpu
def test_gpu_more_chunks_than_blocks(engine):
    case, want = bc.grid_stride()
    bc.assert_same(bc.run_device(engine, case, DEV), want, case.name)


@pytest.mark.gpu
def test_gpu_fuzz(engine):
    import torch

    (d, o, c, fl), programs, results, _ = bc.fuzz()
    first = bc.fuzz_case(d, o, c, fl, programs[0], 0)
    raw = torch.zeros(len(d) + 32, dtype=torch.uint8, device=DEV)
    lead = (first.misalign - raw.data_ptr()) % 16
    data = raw[lead: lead + len(d)]
    data.copy_(torch.from_numpy(d))
    src = (data, torch.from_numpy(o.view(np.int64)).to(DEV), torch.from_numpy(c.view(np.int32)).to(DEV), len(d))
    for j, (p, want) in enumerate(zip(programs, results)):
        bc.assert_same(bc.run_device(engine, bc.fuzz_case(d, o, c, fl, p, j), DEV, source=src), want, f"fuzz{j}")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["synth", "example"])
def test_gpu_real_filter_equals_the_parse_predicate(engine, real_batches, which):
    from pcapplusplus_amd.engine import bpf_on_device, parse_on_device_ex

    b = real_batches[which]
    rec = parse_on_device_ex(engine, b, abi.make_opts(0, 8, False, 8), DEV, tuples=True)
    tup, lay = rec["tuples"], rec["layers"]
    port = PORT if which == "synth" else example_port(tup)
    keep = coincide(b, tup, lay)
    assert keep.sum() > 0.9 * b.n
    matched, bucket, ret, tot = bpf_on_device(engine, b, [bpf.tcp_dst_port(port)], device=DEV)
    want = predicate(tup, port)
    assert want[keep].sum() > 5
    assert np.array_equal(matched[keep] != 0, want[keep])
    ref = bc.run_reference(bc.as_case(which, b, [bpf.tcp_dst_port(port)], frame_lens=b.frame_lens))
    assert np.array_equal(matched, ref.matched[:b.n]) and np.array_equal(bucket, ref.bucket[:b.n])
    assert np.array_equal(ret, ref.ret[:b.n]) and tot == abi.bpf_totals_dict(ref.totals)


def _device_verdicts(engine, case, stream=None):
    """The case's verdict columns as device tensors (left on the device), its source tensors and the loaded filter."""
    import torch

    up = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    data, offs, caps = up(case.data), up(case.offsets.view(np.int64)), up(case.caplens.view(np.int32))
    n = case.n
    matched = torch.full((n,), bc.FILL, dtype=torch.uint8, device=DEV)
    bucket = torch.full((n,), bc.FILL, dtype=torch.uint8, device=DEV)
    totals = torch.zeros(abi.BPF_TOTALS, dtype=torch.int64, device=DEV)
    flt = engine.bpf_load(case.programs)
    st = torch.cuda.current_stream(DEV).cuda_stream if stream is None else stream
    engine.bpf_device(flt, data, offs, caps, n, 1, totals, matched, bucket, None, None, st, data_len=case.dlen())
    return (data, offs, caps, case.dlen()), matched, bucket, flt


@pytest.mark.gpu
def test_gpu_matched_feeds_select(engine):
    """bpf -> select on one stream, nothing read back in between: matched[] is select's keep[]."""
    import torch

    case = BY_NAME["programs_3"]
    ref = bc.run_reference(case)
    sel = sc.Case("bpf_keep", case.data, case.offsets, case.caplens, keep=ref.matched[:case.n].copy())
    want = sc.run_reference(sel)
    src, matched, _, flt = _device_verdicts(engine, case)
    host = sc.alloc(sel)
    up = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    d_data, d_off, d_cap = up(host.data), up(host.offsets.view(np.int64)), up(host.caplens.view(np.int32))
    d_idx, d_tot = up(host.index.view(np.int32)), up(host.totals.view(np.int64))
    engine.select_device(src[0], src[1], src[2], case.n, 1, abi.make_select_spec(keep=abi.ptr(matched)), d_off, d_cap,
                         d_tot, sel.maxp(), d_data, sel.cap(), d_idx, torch.cuda.current_stream(DEV).cuda_stream,
                         data_len=src[3])
    torch.cuda.synchronize(DEV)
    flt.free()
    dn = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
    got = sc.Buffers(dn(d_data, np.uint8), dn(d_off, np.uint64), dn(d_cap, np.uint32), dn(d_idx, np.uint32),
                     dn(d_tot, np.uint64))
    sc.assert_same(got, want, "bpf -> select")
    assert int(want.totals[abi.SEL_SELECTED_PACKETS]) == int(ref.totals[abi.BPF_MATCHED]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("P", [3, 16])
def test_gpu_bucket_feeds_steer(engine, P):
    """bpf -> steer on one stream: bucket[] is steer's column with n_buckets = P, and 0xFF is "not steered"."""
    import torch

    case = BY_NAME[f"programs_{P}"]
    ref = bc.run_reference(case)
    col = ref.bucket[:case.n].copy()
    st = tc.Case("bpf_bucket", case.data, case.offsets, case.caplens, n_buckets=P, bucket=col)
    want = tc.run_reference(st)
    src, _, bucket, flt = _device_verdicts(engine, case)
    run = tc.DeviceRun(replace(st, bucket=np.full(case.n, 0xEE, np.uint8)), DEV, source=src)
    run.rule = bucket  # the column pcppx_bpf_device wrote, still on the device
    run.launch(engine, torch.cuda.current_stream(DEV).cuda_stream)
    got = run.result()
    flt.free()
    tc.assert_same(got, want, "bpf -> steer")
    assert int(want.totals[abi.STEER_DROPPED]) == int((col == 0xFF).sum())
    assert int(want.totals[abi.STEER_STEERED_PACKETS]) == int(ref.totals[abi.BPF_MATCHED])
    if P == 3:
        assert int(want.totals[abi.STEER_DROPPED]) > 100


@pytest.mark.gpu
def test_gpu_two_calls_on_two_streams_agree(engine):
    import torch

    case = BY_NAME["n1000"]
    want = bc.run_reference(case)
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    flt = engine.bpf_load(case.programs)
    try:
        a = bc.run_device(engine, case, DEV, stream=s1, flt=flt)
        b = bc.run_device(engine, case, DEV, stream=s2, flt=flt)
        # and queued together, before either is waited for
        up = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
        data, offs, caps = up(case.data), up(case.offsets.view(np.int64)), up(case.caplens.view(np.int32))
        outs = []
        torch.cuda.synchronize(DEV)
        for s in (s1, s2):
            m = torch.full((case.n,), bc.FILL, dtype=torch.uint8, device=DEV)
            t = torch.zeros(abi.BPF_TOTALS, dtype=torch.int64, device=DEV)
            outs.append((m, t))
        torch.cuda.synchronize(DEV)
        for s, (m, t) in zip((s1, s2), outs):
            engine.bpf_device(flt, data, offs, caps, case.n, 1, t, m, None, None, None, s.cuda_stream)
        torch.cuda.synchronize(DEV)
    finally:
        flt.free()
    bc.assert_same(a, want, "stream 1")
    bc.assert_same(b, want, "stream 2")
    for m, t in outs:
        assert np.array_equal(m.cpu().numpy(), want.matched[:case.n])
        assert t.cpu().numpy().view(np.uint64).tolist() == want.totals.tolist()


# ---------------------------------------------------------------- GPU: packets on both sides of offset 2^32
WIDE_STAGES = ("edges", "edge_plus1", "start_minus1/IPv4/TCP", "end_plus1/IPv6/UDP", "sparse", "tile1500", "bad_desc")


@pytest.mark.gpu
def test_gpu_packets_on_both_sides_of_4gib(engine):
    """One allocation of 2^32 + 2^27 bytes, of which only the stages' extents are written: a program that loads the
    first and the last byte of every packet, and the tcp filter, equal the reference over the same packets in a small
    buffer -- across the offset line, across the address line, and for the bad descriptors of a data_len above 2^32."""
    import torch

    try:
        raw = torch.empty(wc.RAW_BYTES, dtype=torch.uint8, device=DEV)
    except Exception as e:  # no skip for "too big"
        pytest.fail(f"cannot allocate the wide source of {wc.RAW_BYTES} bytes (2^32 + 2^27): {e}")
    try:
        lay = wc.layout(raw.data_ptr(), 5)
        data = raw[lay.pad: lay.pad + lay.data_len]
        stages = {s.name: s for s in wc.stages(lay)}
        bad = straddle = above = 0
        for name in WIDE_STAGES:
            st = stages[name]
            for off, a in st.extents:
                data[off:off + len(a)] = torch.from_numpy(a).to(DEV)
            src = (data, torch.from_numpy(st.offsets.view(np.int64)).to(DEV),
                   torch.from_numpy(st.caplens.view(np.int32)).to(DEV), lay.data_len)
            b = st.compact
            for progs in ([bc.P_ENDS], [bpf.tcp_dst_port(80), bc.P_MIX]):
                case = bc.Case(f"wide {name}", b.data, b.offsets, b.caplens, progs)
                want = bc.run_reference(case)
                bc.assert_same(bc.run_device(engine, case, DEV, source=src), want, case.name)
            bad += int(want.totals[abi.BPF_BAD_DESC])
            straddle += sum(1 for d in st.descs for L in lay.lines if wc.straddles(d, L))
            above += sum(1 for d in st.descs if d.off >= wc.LINE and wc.in_bounds(d.off, d.cap, lay.data_len))
        assert bad >= 8 and straddle >= 6 and above >= 100
    finally:
        del raw, data
        torch.cuda.empty_cache()
