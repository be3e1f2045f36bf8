"""Classic BPF programs for pcppx_bpf_load / pcppx_bpf_device: the opcode constants of <pcap/bpf.h>, an instruction
helper and a reader of `tcpdump -dd` / `-ddd` output.

The engine interprets programs; it does not compile filter strings (libpcap's pcap_compile does, on the caller's side).
A filter compiled elsewhere is pasted in as text:

    prog = bpf.parse_dd(open("filter.dd").read())      # tcpdump -dd 'tcp dst port 443' > filter.dd
    matched, bucket, ret, totals = bpf_on_device(eng, batch, [prog])
"""
from __future__ import annotations

import re

import numpy as np

from .abi import BPF_INSN_DTYPE, BPF_MAX_INSNS, BPF_MAX_PROGRAMS, BPF_MEMWORDS  # noqa: F401

INSN_DTYPE = BPF_INSN_DTYPE  # code u16, jt u8, jf u8, k u32: struct bpf_insn

# instruction classes
LD, LDX, ST, STX, ALU, JMP, RET, MISC = 0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07
# ld / ldx: size and mode
W, H, B = 0x00, 0x08, 0x10
IMM, ABS, IND, MEM, LEN, MSH = 0x00, 0x20, 0x40, 0x60, 0x80, 0xA0
# alu / jmp: operation and operand
ADD, SUB, MUL, DIV, OR, AND, LSH, RSH, NEG, MOD, XOR = 0x00, 0x10, 0x20, 0x30, 0x40, 0x50, 0x60, 0x70, 0x80, 0x90, 0xA0
JA, JEQ, JGT, JGE, JSET = 0x00, 0x10, 0x20, 0x30, 0x40
K, X = 0x00, 0x08
# ret: the value; misc: the transfer
A = 0x10
TAX, TXA = 0x00, 0x80


def insn(code: int, jt: int = 0, jf: int = 0, k: int = 0) -> tuple[int, int, int, int]:
    """One instruction, as BPF_STMT(code, k) / BPF_JUMP(code, k, jt, jf) give it."""
    if not (0 <= code <= 0xFFFF and 0 <= jt <= 0xFF and 0 <= jf <= 0xFF and 0 <= k <= 0xFFFFFFFF):
        raise ValueError(f"instruction field out of range: {(code, jt, jf, k)}")
    return (code, jt, jf, k)


def program(insns) -> np.ndarray:
    """(code, jt, jf, k) rows -> an INSN_DTYPE array."""
    return np.array([insn(*row) for row in insns], dtype=INSN_DTYPE)


_DD = re.compile(r"\{\s*(0x[0-9a-fA-F]+|\d+)\s*,\s*(0x[0-9a-fA-F]+|\d+)\s*,\s*(0x[0-9a-fA-F]+|\d+)\s*,"
                 r"\s*(0x[0-9a-fA-F]+|\d+)\s*\}")


def parse_dd(text: str) -> np.ndarray:
    """A compiled filter as `tcpdump -dd` prints it (C initialisers: `{ 0x28, 0, 0, 0x0000000c },` one per line) or as
    `tcpdump -ddd` does (a line with the instruction count, then `code jt jf k` in decimal per line)."""
    rows = [tuple(int(x, 0) for x in m.groups()) for m in _DD.finditer(text)]
    if rows:
        if _DD.sub("", text).strip(" \t\r\n,"):
            raise ValueError("text between the -dd initialisers")
        return program(rows)
    lines = [ln.split() for ln in text.strip().splitlines() if ln.strip()]
    if not lines or len(lines[0]) != 1:
        raise ValueError("neither -dd initialisers nor a -ddd instruction count")
    count = int(lines[0][0])
    if count != len(lines) - 1 or any(len(ln) != 4 for ln in lines[1:]):
        raise ValueError(f"-ddd: {count} instructions announced, {len(lines) - 1} lines of 4 numbers expected")
    return program([tuple(int(x) for x in ln) for ln in lines[1:]])


def format_dd(prog: np.ndarray) -> str:
    """The `tcpdump -dd` text of a program."""
    return "".join(f"{{ 0x{int(i['code']):x}, {int(i['jt'])}, {int(i['jf'])}, 0x{int(i['k']):08x} }},\n" for i in prog)


def format_ddd(prog: np.ndarray) -> str:
    """The `tcpdump -ddd` text of a program."""
    return f"{len(prog)}\n" + "".join(f"{int(i['code'])} {int(i['jt'])} {int(i['jf'])} {int(i['k'])}\n" for i in prog)


def tcp_dst_port(port: int) -> np.ndarray:
    """"IPv4, not a later fragment, TCP, destination port `port`" over untagged Ethernet: what `tcpdump -dd 'ip and tcp
    dst port N'` compiles to. Returns the snap length 262144, else 0."""
    return program([
        insn(LD | H | ABS, k=12),
        insn(JMP | JEQ | K, 0, 8, 0x0800),
        insn(LD | B | ABS, k=23),
        insn(JMP | JEQ | K, 0, 6, 6),
        insn(LD | H | ABS, k=20),
        insn(JMP | JSET | K, 4, 0, 0x1FFF),
        insn(LDX | B | MSH, k=14),
        insn(LD | H | IND, k=16),
        insn(JMP | JEQ | K, 0, 1, port),
        insn(RET | K, k=262144),
        insn(RET | K, k=0),
    ])
