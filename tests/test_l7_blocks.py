"""The base kernels' second step: dns, http, ssl and sip over more than 64 blocks (the four *_base_kernel).

A block takes 1024 source packets and the base kernel scans 64 blocks' sums a step, with a running carry into the next
step. The four suites stop at 2,049 packets (3 blocks), so the carry is first used here: one case per operator of
66,561 packets (66 blocks, 65 of them full), built by the suite's own builders, in which block 64 holds messages. Their
first record, byte and (sip) SDP positions are the carry of the first 64 blocks plus nothing else, so a carry that is
lost or taken twice moves every record of blocks 64 and 65.

CPU: the reference equals the model on the case, block 64 holds a message, every scanned total is non-zero, and the
totals are the frozen figures below. GPU: the device call equals the reference, whole buffers, the 0xA5 fill included.
"""
from __future__ import annotations

import functools

import pytest

import dns_cases
import http_cases
import sip_cases
import ssl_cases
from pcapplusplus_amd import abi

N = 66561    # 65 blocks of 1024 and one packet
STEP = 64    # blocks a step of the base kernel
BLOCK = 1024

# per operator: the suite, its packets, MSG, the totals' names, the scanned totals and what they come to
OPS = {
    "dns": (dns_cases, lambda: dns_cases.mixed(N, 1), abi.DNS_MSG, abi.dns_totals_dict,
            {"msgs": 687, "rrs": 2247, "name_bytes": 38405}),
    "http": (http_cases, lambda: http_cases.mixed(N, 1), abi.HTTP_MSG, abi.http_totals_dict,
             {"msgs": 688, "fields": 1470, "text_bytes": 27058}),
    "ssl": (ssl_cases, lambda: ssl_cases.mixed(N, 1), abi.SSL_MSG, abi.ssl_totals_dict,
            {"msgs": 816, "hellos": 622, "name_bytes": 20540}),
    "sip": (sip_cases, lambda: sip_cases.mixed(N, "1in100"), abi.SIP_MSG, abi.sip_totals_dict,
            {"msgs": 666, "fields": 2725, "text_bytes": 71565, "sdps": 208}),
}


@functools.lru_cache(maxsize=None)
def wide(op: str):
    """(the case, what the reference leaves): built once, shared by the CPU and the GPU test, never written to."""
    suite, packets = OPS[op][:2]
    case = suite.make("wide", packets())
    return case, suite.run_reference(case)


@pytest.mark.parametrize("op", sorted(OPS))
def test_reference_past_64_blocks(op):
    suite, _, msg, totals_dict, scanned = OPS[op]
    case, want = wide(op)
    assert case.n == N and (N + BLOCK - 1) // BLOCK == STEP + 2
    suite.assert_same(want, suite.model(case), f"{op} wide")
    totals = totals_dict(want.totals)
    assert totals["overflow"] == 0 and totals["host_n"] == 0 and totals["bad_desc"] == 0
    disp = want.disposition[:N]
    assert int((disp[STEP * BLOCK:(STEP + 1) * BLOCK] == msg).sum()) >= 1, "block 64 holds no message"
    assert int((disp[:STEP * BLOCK] == msg).sum()) >= 1, "blocks 0..63 hold no message: block 64's carry would be 0"
    # the frozen figures; none of them is zero, so every scanned carry is exercised
    assert all(v != 0 for v in scanned.values()) and {k: totals[k] for k in scanned} == scanned


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(OPS))
def test_gpu_device_past_64_blocks(engine, op):
    suite = OPS[op][0]
    case, want = wide(op)
    suite.assert_same(suite.run_device(engine, case), want, f"{op} wide")
