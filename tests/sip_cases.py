"""Case generators and runners for pcppx_sip_device / pcppx_sip_reference (tests/test_sip.py).

A Case is a source batch, its parse records (an input: written here the way the parse writes them -- the chain stops at
the TCP / UDP layer with PCPPX_F_NEEDS_HOST_L7 | L7_KNOWN where the ports or the four-byte SIP test trigger a dissector --,
taken from the parse's restatement, or crafted), the spec and the output's capacities. Three runners produce the same
Buffers from it -- model() (pcapplusplus_amd.sip.model, the contract in plain Python), run_reference()
(pcppx_sip_reference) and run_device() (pcppx_sip_device) -- every buffer pre-filled with 0xA5 and over-allocated, so
equality of the whole buffers also shows that nothing beyond the output was touched, and nothing at all but the totals
on overflow.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field, replace

import numpy as np

from pcapplusplus_amd import abi
from pcapplusplus_amd import sip as sp
from pcapplusplus_amd.pcap import from_packets

BLOCK = 1024  # source packets per block of the kernels (pcppx_internal.h kSipBlockPk)
ML = 6        # max_layers of the cases' records, unless a case says otherwise
FILL, F64 = 0xA5, 0xA5A5A5A5A5A5A5A5
PAD_BYTES, PAD_ENTRIES = 64, 4
ETH = abi.LINKTYPE_ETHERNET
NONE, MSG, HOST, BAD = abi.SIP_NONE, abi.SIP_MSG, abi.SIP_HOST, abi.SIP_BAD_DESC
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
SHARES = ("all", "1in100", "last")  # every packet; one in 100; a single message in the last slot of the last block
NAMES = abi.SIP_CALL_NAMES
KNOWN = abi.F_NEEDS_HOST_L7 | abi.F_L7_KNOWN


@dataclass
class Case:
    name: str
    data: np.ndarray      # u8
    offsets: np.ndarray   # u64
    caplens: np.ndarray   # u32
    summary: np.ndarray   # SUMMARY_DTYPE[n]: flags and n_layers are read
    layers: np.ndarray    # LAYER_DTYPE[n, ml]
    ml: int = ML
    names: tuple = NAMES
    fields: int = abi.HTTP_FIELDS_WANTED
    text: int = 3
    kinds: int = 3
    max_msgs: int = 0               # the spec's
    out_msgs: int | None = None     # None: n
    out_fields: int | None = None   # None: exactly what the records need
    out_sdps: int | None = None     # None: exactly what the SDP records need
    text_cap: int | None = None     # None: exactly what the text needs
    want_text: bool = True
    want_disp: bool = True
    use_brief: bool = False
    data_len: int | None = None
    meta: dict = field(default_factory=dict)

    @property
    def n(self) -> int:
        return len(self.caplens)

    def dlen(self) -> int:
        return len(self.data) if self.data_len is None else self.data_len

    def maxm(self) -> int:
        return self.n if self.out_msgs is None else self.out_msgs

    def maxf(self) -> int:
        return int(needs(self)[1]) if self.out_fields is None else self.out_fields

    def maxs(self) -> int:
        return int(needs(self)[3]) if self.out_sdps is None else self.out_sdps

    def cap(self) -> int:
        return int(needs(self)[2]) if self.text_cap is None else self.text_cap


@dataclass
class Buffers:
    msgs: np.ndarray               # u8: (out_msgs + PAD_ENTRIES) * 48 bytes
    fields: np.ndarray             # u8: (out_fields + PAD_ENTRIES) * 24 bytes
    sdps: np.ndarray               # u8: (out_sdps + PAD_ENTRIES) * 32 bytes
    text: np.ndarray | None        # u8
    disposition: np.ndarray | None
    totals: np.ndarray

    def messages(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.SIP_MSGS]) if k is None else k
        return self.msgs[:k * 48].view(abi.SIP_MSG_DTYPE)

    def records(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.SIP_FIELDS]) if k is None else k
        return self.fields[:k * 24].view(abi.SIP_FIELD_DTYPE)

    def bodies(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.SIP_SDPS]) if k is None else k
        return self.sdps[:k * 32].view(abi.SIP_SDP_DTYPE)

    def the_text(self) -> np.ndarray:
        return self.text[:int(self.totals[abi.SIP_TEXT_BYTES])]

    def rows(self) -> list[tuple]:
        return sp.rows(self.messages(), self.records(), self.the_text())

    def calls(self, names=NAMES) -> dict:
        return sp.calls(self.messages(), self.records(), self.bodies(), self.the_text(), names)


FIELDS = ("msgs", "fields", "sdps", "text", "disposition")


def alloc(c: Case) -> Buffers:
    return Buffers(np.full((c.maxm() + PAD_ENTRIES) * 48, FILL, np.uint8),
                   np.full((c.maxf() + PAD_ENTRIES) * 24, FILL, np.uint8),
                   np.full((c.maxs() + PAD_ENTRIES) * 32, FILL, np.uint8),
                   np.full(c.cap() + PAD_BYTES, FILL, np.uint8) if c.want_text else None,
                   np.full(c.n + PAD_ENTRIES, FILL, np.uint8) if c.want_disp else None,
                   np.full(abi.SIP_TOTALS, F64, np.uint64))


# ------------------------------------------------------------------ runners
_MODEL: dict[tuple, tuple] = {}


def _result(c: Case, **kw) -> sp.Result:
    return sp.model(c.data, c.offsets, c.caplens, c.dlen(), c.summary["flags"], c.summary["n_layers"], c.layers, c.ml,
                    c.names, c.fields, c.text, c.kinds, **kw)


def needs(c: Case) -> tuple[int, int, int, int]:
    """(messages, records, text bytes, SDP records) of the case's spec over its batch, whatever its capacities. The
    model runs once per batch and spec; every case made from it with replace() shares the answer."""
    key = (id(c.data), id(c.offsets), id(c.caplens), id(c.layers), id(c.summary), c.ml, c.names, c.fields, c.text,
           c.kinds, c.data_len)
    if key not in _MODEL:
        r = _result(c)
        _MODEL[key] = (len(r.msgs), len(r.fields), len(r.text), len(r.sdps), c)  # c kept alive: the ids stay its own
    return _MODEL[key][:4]


def model(c: Case) -> Buffers:
    """include/pcppx.h's sip contract, restated in pcapplusplus_amd/sip.py, as the buffers a call leaves."""
    out = alloc(c)
    r = _result(c, max_msgs=c.max_msgs, out_msgs=c.maxm(), out_fields=c.maxf(), out_sdps=c.maxs(), text_cap=c.cap(),
                want_text=c.want_text)
    out.totals[:] = r.totals
    if r.disposition is None:
        return out
    if out.disposition is not None:
        out.disposition[:c.n] = r.disposition
    out.msgs[:len(r.msgs) * 48] = sp.msgs_array(r.msgs).view(np.uint8)
    out.fields[:len(r.fields) * 24] = sp.fields_array(r.fields).view(np.uint8)
    out.sdps[:len(r.sdps) * 32] = sp.sdps_array(r.sdps).view(np.uint8)
    if out.text is not None:
        out.text[:len(r.text)] = np.frombuffer(r.text, np.uint8)
    return out


def spec_of(c: Case) -> abi.SipSpec:
    return abi.make_sip_spec(c.names, c.fields, c.text, c.kinds, c.max_msgs)


def brief_of(c: Case) -> np.ndarray:
    rec = np.zeros(max(c.n, 1), abi.BRIEF_DTYPE)
    for f in abi.BRIEF_DTYPE.names:
        rec[f][:c.n] = c.summary[f]
    return rec


def run_reference(c: Case) -> Buffers:
    out = alloc(c)
    data = c.data if len(c.data) else np.zeros(1, np.uint8)
    b = abi.Batch(data.ctypes.data, c.offsets.ctypes.data, c.caplens.ctypes.data, c.dlen(), c.n, ETH, 0)
    lay = np.ascontiguousarray(c.layers) if c.n else np.zeros((1, c.ml), abi.LAYER_DTYPE)
    if c.use_brief:
        rec = brief_of(c)
        r = abi.Records(None, lay.ctypes.data)
        r.brief = rec.ctypes.data
    else:
        rec = np.ascontiguousarray(c.summary) if c.n else np.zeros(1, abi.SUMMARY_DTYPE)
        r = abi.Records(rec.ctypes.data, lay.ctypes.data)
    opt = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    o = abi.SipOut(out.msgs.ctypes.data, out.fields.ctypes.data, out.sdps.ctypes.data, opt(out.text), c.cap(),
                   opt(out.disposition), c.maxm(), c.maxf(), c.maxs(), 0, out.totals.ctypes.data)
    abi.sip_reference(b, r, c.ml, spec_of(c), o)
    del rec, lay
    return out


class DeviceRun:
    """A case's tensors on the device; launch() queues pcppx_sip_device on a stream, result() reads the buffers."""

    def __init__(self, c: Case, device: str = "cuda:0", source=None):
        """source: (data, offsets, caplens, data_len) tensors already on the device to read from instead of c's own
        batch (c then holds the spec, the records and, for the runners on the host, the same packets in a small
        buffer)."""
        self.c, self.device = c, device
        host = alloc(c)
        if source is None:
            self.data = self.up(c.data if len(c.data) else np.zeros(1, np.uint8))
            self.offsets, self.caplens = self.up(c.offsets.view(np.int64)), self.up(c.caplens.view(np.int32))
            self.data_len = c.dlen()
        else:
            self.data, self.offsets, self.caplens, self.data_len = source
        u8 = lambda a: self.up(np.ascontiguousarray(a).view(np.uint8).reshape(-1))  # noqa: E731
        pad = lambda a, dt: a if len(a) else np.zeros(1, dt)  # noqa: E731
        if c.use_brief:
            self.summary, self.brief = None, u8(brief_of(c))
        else:
            self.summary, self.brief = u8(pad(c.summary, abi.SUMMARY_DTYPE)), None
        self.layers = u8(pad(c.layers.reshape(-1), abi.LAYER_DTYPE))
        self.d_msgs, self.d_fields, self.d_sdps = self.up(host.msgs), self.up(host.fields), self.up(host.sdps)
        self.d_text = None if host.text is None else self.up(host.text)
        self.d_disp = None if host.disposition is None else self.up(host.disposition)
        self.d_tot = self.up(host.totals.view(np.int64))

    def up(self, a: np.ndarray):
        import torch

        return torch.from_numpy(a).to(self.device)

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.sip_device(self.data, self.offsets, self.caplens, c.n, ETH, self.layers, c.ml, spec_of(c), self.d_msgs,
                          self.d_fields, self.d_sdps, self.d_tot, c.maxm(), c.maxf(), c.maxs(), self.d_text, c.cap(),
                          self.d_disp, stream, data_len=self.data_len, summary=self.summary, brief=self.brief)

    def result(self) -> Buffers:
        import torch

        torch.cuda.synchronize(self.device)
        down = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return Buffers(down(self.d_msgs), down(self.d_fields), down(self.d_sdps), down(self.d_text),
                       down(self.d_disp), down(self.d_tot).view(np.uint64))


def run_device(engine, c: Case, device: str = "cuda:0", source=None) -> Buffers:
    import torch

    run = DeviceRun(c, device, source)
    run.launch(engine, torch.cuda.current_stream(device).cuda_stream)
    return run.result()


def assert_same(got: Buffers, want: Buffers, what: str) -> None:
    """Whole buffers, pads included: the written part equal, the 0xA5 fill intact everywhere else."""
    assert list(got.totals) == list(want.totals), (what, "totals", list(got.totals), list(want.totals))
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        assert (g is None) == (w is None), (what, f)
        if g is None:
            continue
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.nonzero(g != w)[0]
        assert len(bad) == 0, (what, f, len(bad), "first at", int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def assert_untouched(got: Buffers, what: str) -> None:
    """The all-or-nothing rule: the records, the text and the dispositions still hold the fill."""
    for f in FIELDS:
        g = getattr(got, f)
        assert g is None or bool((g == FILL).all()), (what, f)


# ------------------------------------------------------------------ records
L7_PORTS = frozenset((53, 5353, 5355, 67, 68)) | sp.GATED_EITHER | frozenset((5060, 5061))


def chain_of(pkt: bytes) -> tuple[list, int]:
    """The chain and the flags the parse records for a packet of sp.packet(): (proto, osi, offset, hdr_len, data_len)
    per layer. A payload whose ports, or on UDP whose first four bytes, trigger an L7 dissector stops the chain at the L4
    layer with NEEDS_HOST_L7 (| L7_KNOWN | L7_DNS as the parse names it); any other payload is a generic layer (proto
    32 here) behind it."""
    n = len(pkt)
    tcp = pkt[23] == 6
    at = 54 if tcp else 42
    chain = [(1, 2, 0, 14, n), (2, 3, 14, 20, n - 14), (sp.P_TCP if tcp else sp.P_UDP, 4, 34, at - 34, n - 34)]
    left = n - at
    if left <= 0:
        return chain, 0
    sport, dport = int.from_bytes(pkt[34:36], "big"), int.from_bytes(pkt[36:38], "big")
    trig = sport in L7_PORTS or dport in L7_PORTS or dport == 4789 or (not tcp and left >= 4 and pkt[at:at + 4] in sp.KEYS)
    if not trig:
        return chain + [(32, 7, at, left, left)], 0
    if not tcp:
        dhcp = (sport, dport) in ((68, 67), (67, 68), (67, 67))
        if not dhcp and dport != 4789 and left >= 12 and (sport in (53, 5353, 5355) or dport in (53, 5353, 5355)):
            return chain, KNOWN | abi.F_L7_DNS
        if dport == 4789 or 2152 in (sport, dport) or 2123 in (sport, dport):
            return chain, abi.F_NEEDS_HOST_L7
    return chain, KNOWN


def make(name: str, packets: list[bytes], chains: list | None = None, flags: list | None = None, ml: int = ML,
         n_layers: list | None = None, **kw) -> Case:
    """A case over the packets back to back. chains[i]: packet i's layer entries (None: chain_of it), of which the
    first ml are recorded; flags[i] (None: chain_of's, or DEPTH_OVERFLOW past ml); n_layers[i] (None: the chain's length
    capped at ml, as the parse caps it)."""
    n = len(packets)
    caps = np.array([len(p) for p in packets], np.uint32)
    offs = (np.cumsum(caps, dtype=np.uint64) - caps).astype(np.uint64)
    data = np.frombuffer(b"".join(packets) + b"\0", np.uint8).copy()
    summary = np.zeros(n, abi.SUMMARY_DTYPE)
    layers = np.zeros((n, ml), abi.LAYER_DTYPE)
    for i, p in enumerate(packets):
        chain, fl = chain_of(p)
        if chains is not None and chains[i] is not None:
            chain = chains[i]
        for k, e in enumerate(chain[:ml]):
            layers[i, k] = e
        summary["n_layers"][i] = min(len(chain), ml) if n_layers is None or n_layers[i] is None else n_layers[i]
        fl |= abi.F_DEPTH_OVERFLOW if len(chain) > ml else 0
        summary["flags"][i] = fl if flags is None or flags[i] is None else flags[i]
    return Case(name, data, offs, caps, summary, layers, ml=ml, **kw)


def parsed(name: str, packets: list[bytes], opts=None, **kw) -> Case:
    """A case whose records are the parse's own, through its restatement (oracle.oracle_parse)."""
    import oracle

    opts = opts or abi.make_opts()
    b = from_packets(packets)
    summary, layers = oracle.oracle_parse(b, opts)
    return Case(name, np.concatenate([b.data, np.zeros(1, np.uint8)]), b.offsets, b.caplens, summary,
                np.ascontiguousarray(layers).reshape(b.n, opts.max_layers), ml=opts.max_layers,
                data_len=int(b.caplens.sum()), **kw)


# ------------------------------------------------------------------ packets
SDP = sp.sdp_body("192.168.1.20", 49170, 51372)
INVITE = sp.request("INVITE", "sip:bob@biloxi.example.com", sp.dialog_headers(1, SDP, True), SDP)
OK200 = sp.response(200, "OK", sp.dialog_headers(2, SDP, True), SDP)


def on_port(payload: bytes, k: int = 0, **kw) -> bytes:
    return sp.packet(payload, k, **kw)


def off_port(payload: bytes, k: int = 0, **kw) -> bytes:
    """UDP between two ports that gate nothing: the heuristic path."""
    return sp.packet(payload, k, sport=40000 + k % 1000, dport=6000 + k % 7, **kw)


def _req(m: str, k: int) -> bytes:
    return sp.request(m, f"sip:u{k}@example.com", sp.dialog_headers(k))


# rule 7, requests: (name, payload); every payload goes out on the port path over UDP and TCP and on the heuristic path
METHOD_LINES = [(f"method_{m}", _req(m, k)) for k, m in enumerate(abi.SIP_METHODS)]
NEAR_MISSES = [(f"{kind}_{m}", p) for m in abi.SIP_METHODS for kind, p in (
    ("lower", f"{m.lower()} sip:a@b SIP/2.0\r\n\r\n".encode()),
    ("no_space", f"{m}sip:a@bSIP/2.0".encode()),
    ("space_at_0", f" {m} sip:a@b SIP/2.0\r\n\r\n".encode()),
    ("longer", f"{m}X sip:a@b SIP/2.0\r\n\r\n".encode()),
    ("shorter", f"{m[:-1]} sip:a@b SIP/2.0\r\n\r\n".encode()))]
REQUEST_LINES = [
    ("L_3", b"BYE"),
    ("L_4_space_last", b"BYE "),
    ("L_4_no_space", b"INFO"),
    ("no_version", b"INVITE sip:bob@example.com\r\nVia: x\r\n\r\n"),
    ("no_version_no_newline", b"INVITE sip:bob@example.com"),
    ("cut_v_plus_5", b"INVITE sip:b SIP/"),
    ("cut_v_plus_6", b"INVITE sip:b SIP/2"),
    ("cut_v_plus_7", b"INVITE sip:b SIP/2."),
    ("cut_v_plus_8", b"INVITE sip:b SIP/2.0"),
    ("cut_inside_sip", b"INVITE sip:b SIP"),
    ("empty_uri", b"INVITE  SIP/2.0\r\nVia: x\r\n\r\n"),
    ("uri_with_spaces", b"REFER sip:a b c SIP/2.0\r\n\r\n"),
    ("two_versions", b"ACK sip:a SIP/1.0 SIP/2.0\r\n\r\n"),
    ("version_in_header", b"BYE sip:a\r\nX: y SIP/2.0\r\nZ: 1\r\n\r\n"),
    ("lf_only", b"OPTIONS sip:a SIP/2.0\nVia: x\n\n"),
    ("short_version", b"INVITE sip:b SIP/2\r\nVia: x\r\n\r\n"),
    ("version_6_bytes", b"NOTIFY sip:b SIP/2.\r\n\r\n"),
    ("http_version", b"INVITE sip:b HTTP/1.1\r\nVia: x\r\n\r\n"),
    ("no_second_space", b"INVITE sip:bob@example.com\r\n"),
    ("almost_sip", b"UPDATE sip:b SIP SIP/ SIP/2.0\r\n\r\n"),
    ("version_then_cr_only", b"PRACK sip:b SIP/2.0\rVia: x\r\n\r\n"),
    ("key_but_unknown_method", b"INVITED sip:b SIP/2.0\r\n\r\n"),
]
LAST_BYTES = (0x0A, 0x00, 0x0D, 0x20, 0xFF)  # the carrier header's last byte, before a request without " SIP/"


def _res(code: bytes, rest: bytes = b" OK\r\nVia: x\r\n\r\n", version: bytes = b"SIP/2.0") -> bytes:
    return version + b" " + code + rest


CODE_LINES = [(f"code_{c}", sp.response(c, "Text", sp.dialog_headers(c))) for c in sorted(sp.CODES)]
REJECTED = [(f"rejected_{c}", sp.response(c, "No")) for c in (99, 101, 179, 184, 198, 201, 299, 306, 418, 499, 514,
                                                                  599, 601, 605, 609, 700, 999)]
RESPONSE_LINES = [
    ("ok", _res(b"200")),
    ("L_11", b"SIP/2.0 200"),
    ("L_12", b"SIP/2.0 200 "),
    ("L_13", b"SIP/2.0 200 O"),
    ("L_14_cr", b"SIP/2.0 200 \r\n"),
    ("no_space_at_11", b"SIP/2.0 2000 OK\r\n\r\n"),
    ("not_digits", _res(b"2x0")),
    ("letters", _res(b"abc")),
    ("wraps_to_100", _res(b"5\n\x1c")),        # 500 - 380 - 20
    ("wraps_to_200_high", _res(b"2:\xcc")),    # 200 + 100 - 100, a byte >= 0x80
    ("high_bytes", _res(b"\x80\x90\xa0")),
    ("no_newline", b"SIP/2.0 180 Ringing and on"),
    ("no_newline_cr_before_end", b"SIP/2.0 180 Ringing\rx"),
    ("resp_lf_only", b"SIP/2.0 404 Not Found\nVia: x\n\n"),
    ("newline_inside_version", b"SIP/2.\n 200 OK\r\n\r\n"),
    ("not_sip", b"XIP/2.0 200 OK\r\nVia: x\r\n\r\n"),
    ("long_version", b"SIP/2.0xxxx 200 OK\r\n\r\n"),
    ("no_space_at_all", b"SIP/2.0/200/OK/and/more"),
    ("s_plus_4_at_L_minus_1", b"SIP/2.0xxxx 200 "),
    ("s_plus_4_at_L", b"SIP/2.0xxxx 200"),
    ("s_plus_4_at_L_plus_1", b"SIP/2.0xxxx 20"),
    ("s_plus_4_far", b"SIP/2.0xxxxxxx "),
    ("heuristic_bad_code", b"SIP/2.0xxxx 299 OK\r\n\r\n"),
    ("heuristic_no_space_behind_code", b"SIP/2.0xxxx 2000 OK\r\n"),
    ("version_6", b"SIP/2. 200 OK\r\n\r\n"),
]


def lines() -> list[bytes]:
    """Every first line on the UDP port path, the TCP port path and the heuristic path; the requests without " SIP/"
    behind every LAST_BYTES value."""
    out, k = [], 0
    for _, p in METHOD_LINES + NEAR_MISSES + REQUEST_LINES + CODE_LINES + REJECTED + RESPONSE_LINES:
        out += [on_port(p, k), on_port(p, k + 1, tcp=True), off_port(p, k + 2)]
        k += 3
    for last in LAST_BYTES:
        for name in ("no_version", "no_version_no_newline", "cut_v_plus_6", "cut_inside_sip"):
            p = dict(REQUEST_LINES)[name]
            out += [on_port(p, k, last=last), on_port(p, k + 1, tcp=True, last=last)]
            k += 2
    return out


# rule 5: (name, sport, dport); each with a request key, the response key and no key
PORTS = [("dhcp_68_67", 68, 67), ("dhcp_67_68", 67, 68), ("dhcp_67_67", 67, 67), ("not_dhcp_68_68", 68, 68),
         ("vxlan_dst", 40000, 4789), ("vxlan_src", 4789, 40000), ("dhcp_and_sip", 67, 67), ("sip_src", 5060, 40000),
         ("sips_dst", 40000, 5061), ("sip_and_vxlan", 5060, 4789), ("dns_dst", 40000, 53), ("dns_src", 53, 40000),
         ("plain", 40000, 6000)] + \
    [(f"gated_dst_{p}", 40000, p) for p in sorted(sp.GATED_EITHER | sp.GATED_DST)] + \
    [(f"gated_src_{p}", p, 40000) for p in sorted(sp.GATED_EITHER | sp.GATED_DST)]
PORT_PAYLOADS = (INVITE, OK200, b"BYE a SIP/2.0", b"SIP/2.0 200", b"\x00\x01\x02\x03 not sip at all", b"SIP")


def ports() -> tuple[list[bytes], list[int]]:
    """The port cases with KNOWN flags (so that rule 5 itself decides), then again with the parse's own flags."""
    pk = [sp.packet(p, k, sport=s, dport=d) for k, (_, s, d) in enumerate(PORTS) for p in PORT_PAYLOADS]
    pk += [sp.packet(p, k, sport=s, dport=d, tcp=True) for k, (_, s, d) in enumerate(PORTS) for p in PORT_PAYLOADS[:2]]
    return pk + pk, [KNOWN] * len(pk) + [None] * len(pk)


def _with(headers: list, body: bytes = SDP, first: bytes = b"INVITE sip:bob@example.com SIP/2.0\r\n") -> bytes:
    return first + b"".join(h if isinstance(h, bytes) else f"{h[0]}: {h[1]}\r\n".encode("latin-1")
                            for h in headers) + b"\r\n" + body


CT = ("Content-Type", "application/sdp")
CL = ("Content-Length", str(len(SDP)))
# rules 12 and 13, the header side: (name, payload)
CONTENT_CASES = [
    ("plain", _with([CT, CL])),
    ("length_first", _with([CL, CT])),
    ("compact_l", _with([CT, ("l", str(len(SDP)))])),
    ("negative", _with([CT, ("Content-Length", "-5")])),
    ("zero", _with([CT, ("Content-Length", "0")])),
    ("above_2_31", _with([CT, ("Content-Length", "2147483648")])),
    ("at_2_31_minus_1", _with([CT, ("Content-Length", "2147483647")])),
    ("huge", _with([CT, ("Content-Length", "99999999999999999999999")])),
    ("absent", _with([CT])),
    ("no_value", _with([CT, b"Content-Length:\r\n"])),
    ("two_lengths", _with([CT, ("Content-Length", "0"), CL])),
    ("length_upper", _with([CT, ("CONTENT-LENGTH", "7")])),
    ("type_lower_name", _with([("content-type", "application/sdp"), CL])),
    ("type_upper_value", _with([("Content-Type", "application/SDP"), CL])),
    ("type_in_the_middle", _with([("Content-Type", "multipart/mixed;x=application/sdp;boundary=z"), CL])),
    ("type_cut", _with([("Content-Type", "application/sd"), CL])),
    ("type_behind_nul", _with([b"Content-Type: text/plain\0application/sdp\r\n", CL])),
    ("type_nul_inside", _with([b"Content-Type: application\0/sdp\r\n", CL])),
    ("two_types_first_wins", _with([("Content-Type", "text/plain"), CT, CL])),
    ("two_types_first_sdp", _with([CT, ("Content-Type", "text/plain"), CL])),
    ("type_compact_c", _with([("c", "application/sdp"), CL])),
    ("type_no_value", _with([b"Content-Type:\r\n", CL])),
    ("no_type", _with([CL])),
    ("no_body", _with([CT, CL], b"")),
    ("header_incomplete", b"INVITE sip:b SIP/2.0\r\nContent-Type: application/sdp\r\nContent-Length: 9"),
    ("response_with_sdp", _with([CT, CL], SDP, b"SIP/2.0 183 Session Progress\r\n")),
    ("length_behind_nul", _with([CT, b"Content-Length: 12\0003\r\n"])),
    ("value_behind_nul", _with([b"Call-ID: abc\0def@host\r\n", b"From: \0\r\n", CT, CL])),
    ("nul_ends_last_field", _with([CT, CL])[:-len(SDP) - 2 - 4] + b"\0\0\0\0" + SDP),
    ("first_line_len_0", _with([CT, CL], SDP, b"INVITE sip:bob@example.com\r\n")),
]


def _body(*lines_: bytes, eol: bytes = b"\r\n", last: bool = True) -> bytes:
    return eol.join(lines_) + (eol if last else b"")


O = b"o=alice 1 2 IN IP4 "
# rule 13, the body side: (name, body)
SDP_CASES = [
    ("plain", SDP),
    ("lf_only", sp.sdp_body("10.1.2.3", 4000, 4002, eol=b"\n")),
    ("no_o", _body(b"v=0", b"s=-", b"m=audio 4000 RTP/AVP 0")),
    ("five_tokens", _body(b"v=0", b"o=alice 1 2 IN IP4", b"m=audio 4000 RTP/AVP 0")),
    ("seven_tokens", _body(b"o=alice 1 2 IN IP4 1.2.3.4 extra")),
    ("ip6", _body(b"o=alice 1 2 IN IP6 ::1", b"m=video 6000 RTP/AVP 31")),
    ("not_in", _body(b"o=alice 1 2 in IP4 1.2.3.4")),
    ("in_with_nul", _body(b"o=alice 1 2 IN\0 IP4 1.2.3.4")),
    ("tabs", _body(b"o=alice\t1\t2\tIN\tIP4\t1.2.3.4", b"m=audio\t4000")),
    ("two_o_first_wins", _body(b"o=alice 1 2 IN IP4 1.2.3.4", b"o=alice 1 2 IN IP4 5.6.7.8")),
    ("two_o_first_bad", _body(b"o=alice 1 2 IN IP4 bad", b"o=alice 1 2 IN IP4 5.6.7.8")),
    ("upper_o", _body(b"O=alice 1 2 IN IP4 9.8.7.6", b"M=audio 1234 x")),
    ("o_no_value", _body(b"o=", b"m=audio 5 x")),
    ("o_no_separator_at_end", _body(b"v=0", b"o", last=False)),
    ("o_space_name", _body(b"o =alice 1 2 IN IP4 1.2.3.4")),
    ("space_not_skipped", _body(b"o= alice 1 2 IN IP4 1.2.3.4", b"m= audio 7 x")),
    ("addr_leading_zero", _body(O + b"01.2.3.4")),
    ("addr_zero_octet", _body(O + b"10.0.0.1")),
    ("addr_double_zero", _body(O + b"10.00.0.1")),
    ("addr_three", _body(O + b"1.2.3")),
    ("addr_five", _body(O + b"1.2.3.4.5")),
    ("addr_trailing_dot", _body(O + b"1.2.3.4.")),
    ("addr_leading_dot", _body(O + b".1.2.3.4")),
    ("addr_double_dot", _body(O + b"1..2.3.4")),
    ("addr_256", _body(O + b"256.1.1.1")),
    ("addr_255", _body(O + b"255.255.255.255")),
    ("addr_4_digits", _body(O + b"1.2.3.0004")),
    ("addr_hex", _body(O + b"0x1.2.3.4")),
    ("addr_all_zero", _body(O + b"0.0.0.0")),
    ("addr_nul_tail", _body(O + b"1.2.3.4\0junk")),
    ("addr_nul_head", _body(O + b"\0001.2.3.4")),
    ("addr_letters", _body(O + b"host.example.com")),
    ("addr_no_newline", _body(O + b"7.7.7.7", last=False)),
    ("several_m", _body(b"m=text 1 x", b"m=audio", b"m=video 6000 x", b"m=audio 4000 x", b"m=audio 4002 x",
                        b"m=video 6002 x")),
    ("m_one_token", _body(b"m=audio")),
    ("m_audio_upper", _body(b"m=AUDIO 4000 x")),
    ("m_audio_nul", _body(b"m=audio\0 4000 x", b"m=audio 4\0007 x")),
    ("port_65535", _body(b"m=audio 65535 x", b"m=video 65536 x")),
    ("port_70000", _body(b"m=audio 70000 x", b"m=video -1 x")),
    ("port_huge", _body(b"m=audio 99999999999999999999 x", b"m=video -99999999999999999999 x")),
    ("port_long_max", _body(b"m=audio 9223372036854775807 x", b"m=video 9223372036854775808 x")),
    ("port_long_min", _body(b"m=audio -9223372036854775808 x", b"m=video -9223372036854775809 x")),
    ("port_plus", _body(b"m=audio +80 x", b"m=video +-80 x")),
    ("port_text", _body(b"m=audio 40x00 x", b"m=video x x")),
    ("port_zero", _body(b"m=audio 0 x")),
    ("no_line_end", _body(b"v=0", b"m=audio 4000 RTP/AVP 0", last=False)),
    ("empty_line_ends_it", _body(b"v=0", b"", b"m=audio 4000 x")),
    ("starts_with_newline", b"\r\n" + SDP),
    ("nul_ends_it", b"v=0\r\nm=audio 4000\0 x"),
    ("nul_at_start", b"\0" + SDP),
    ("no_separator_lines", _body(b"v0", b"oalice", b"m=audio 9 x")),
    ("separator_on_a_later_line", b"v\r\no=alice 1 2 IN IP4 1.2.3.4\r\n"),
    ("one_byte", b"m"),
    ("owner_and_video", _body(O + b"1.1.1.1", b"m=video 5 x")),
]


def content() -> list[bytes]:
    out = [on_port(p, k) for k, (_, p) in enumerate(CONTENT_CASES)]
    out += [on_port(_with([CT, ("Content-Length", str(len(b)))], b), 100 + k) for k, (_, b) in enumerate(SDP_CASES)]
    # the first line missing on the port path with 0x0A in front: the request line itself is the first field
    out.append(on_port(dict(CONTENT_CASES)["first_line_len_0"], 99, last=0x0A))
    return out


def sip_k(k: int) -> bytes:
    """SIP packet k of the mixed batches: requests and responses in turn over both paths and carriers, every third with
    an SDP body, a few incomplete or odd."""
    body = sp.sdp_body(f"10.{k % 200}.{k % 7}.{1 + k % 250}", 10000 + 2 * (k % 2000), 20000 + k % 999 if k % 6 == 0 else
                       None) if k % 3 == 0 else b""
    h = sp.dialog_headers(k, body, bool(body))
    if k % 11 == 0:
        h.insert(2, ("Call-ID", "dup@x"))  # a repeated name: only the first is FIRST
    if k % 2 == 0:
        p = sp.request(abi.SIP_METHODS[k % 14], f"sip:user{k}@example.com", h, body, end=k % 17 != 0)
    else:
        code = sorted(sp.CODES)[k % 77]
        p = sp.response(code, "Reason %d" % k, h, body, eol=b"\n" if k % 13 == 0 else b"\r\n")
    p = p[:len(p) - (k % 29 if k % 23 == 0 else 0)]
    if k % 5 == 0:
        return off_port(p, k)
    return on_port(p, k, tcp=k % 7 == 0)


def other_k(k: int) -> bytes:
    """A packet without a SIP layer: an empty TCP ACK, a payload on ports that trigger nothing, a DNS-sized payload."""
    if k % 3 == 0:
        return sp.packet(b"", k, dport=443, tcp=True)
    if k % 3 == 1:
        return sp.packet(bytes(1 + (k + j) % 250 for j in range(20 + k % 30)), k, dport=4000 + k % 10, tcp=k % 2 == 0)
    return sp.packet(bytes((k + j) % 256 for j in range(12 + k % 40)), k, dport=53)


def mixed(n: int, share: str) -> list[bytes]:
    """n packets: all SIP, one in 100, or a single message in the last slot of the last block."""
    if share == "last":
        return [other_k(k) for k in range(n - 1)] + ([on_port(INVITE, 5)] if n else [])
    step = {"all": 1, "1in100": 100}[share]
    return [sip_k(k) if k % step == 0 else other_k(k) for k in range(n)]


FLAG_BITS = (abi.F_NEEDS_HOST_L7, abi.F_NEEDS_HOST_PROTO, abi.F_DEPTH_OVERFLOW, abi.F_OVERSIZE, abi.F_BAD_DESC,
             abi.F_L7_KNOWN, abi.F_L7_SSL, abi.F_L7_HTTP, abi.F_L7_DNS)


def flag_combinations() -> list[int]:
    return [sum(b for j, b in enumerate(FLAG_BITS) if (m >> j) & 1) | (abi.F_IP_CSUM if m % 3 == 0 else 0)
            for m in range(512)]


MUTATION_BYTES = (0x00, 0x0A, 0x0D, 0x20, 0x3A, 0x3D, 0x09, 0x2E, 0x30, 0x39, 0x41, 0x7A, 0x80, 0xFF)


def mutate(m: bytearray, rng, first: int = 0) -> None:
    """One to four seeded changes to the message that starts at m[first]: a random byte, one of the bytes the rules
    look for, a bit flip, or a swap of two bytes."""
    size = len(m) - first
    if size <= 0:
        return
    for _ in range(int(rng.integers(1, 5))):
        at = first + int(rng.integers(size))
        kind = int(rng.integers(4))
        if kind == 0:
            m[at] = int(rng.integers(256))
        elif kind == 1:
            m[at] = MUTATION_BYTES[int(rng.integers(len(MUTATION_BYTES)))]
        elif kind == 2:
            m[at] ^= 1 << int(rng.integers(8))
        else:
            to = first + int(rng.integers(size))
            m[at], m[to] = m[to], m[at]


def fuzz(count: int, seed: int) -> list[bytes]:
    """Seeded mutations of the crafted messages, a third of them cut short, over both paths and carriers."""
    rng = np.random.default_rng(seed)
    base = [p for _, p in METHOD_LINES + REQUEST_LINES + CODE_LINES[::7] + RESPONSE_LINES + CONTENT_CASES] + \
        [_with([CT, ("Content-Length", str(len(b)))], b) for _, b in SDP_CASES]
    out = []
    for k in range(count):
        m = bytearray(base[int(rng.integers(len(base)))])
        mutate(m, rng)
        if len(m) > 1 and rng.integers(3) == 0:
            m = m[:int(rng.integers(1, len(m) + 1))]
        way = int(rng.integers(4))
        last = int(rng.integers(256)) if rng.integers(4) else 0x0A
        out.append(off_port(bytes(m), k, last=last) if way == 0 else on_port(bytes(m), k, tcp=way == 1, last=last))
    return out


# ------------------------------------------------------------------ the frozen answers of the real SIP layers
# tests/golden/sip/expected.npz (tools/make_golden_sip.py writes it, the tests read it): one JSON text per file, a list
# with one entry per packet: null where the reference builds no SIP layer, the string "undefined" where its answer is
# undefined (rule 8), else
#   [kind, getDataLen(), getHeaderLen(), getFieldCount(), isHeaderComplete(), getContentLength(), method, URI or status
#    text as hex, status code as int, getVersion() as hex, the first line's getSize(), its isComplete(),
#    [[name as hex, value as hex], ...], null or [the SdpLayer's getFieldCount(), getOwnerIPv4Address() as 4 bytes hex,
#    getMediaPort("audio"), getMediaPort("video")]]
def save_frozen(path, frozen: dict) -> None:
    files = sorted(frozen)
    np.savez_compressed(path, files=np.array(files),
                        **{f"f{k}": np.frombuffer(json.dumps(frozen[f], separators=(",", ":")).encode(), np.uint8)
                           for k, f in enumerate(files)})


def load_frozen(path) -> dict:
    z = np.load(path, allow_pickle=False)
    return {str(f): json.loads(z[f"f{k}"].tobytes().decode()) for k, f in enumerate(z["files"])}


def crafted_packets() -> list[bytes]:
    """What tools/make_golden_sip.py puts into crafted.pcap ahead of the mutated real packets."""
    return lines() + ports()[0][:len(ports()[0]) // 2] + content() + fuzz(600, 11)


# ------------------------------------------------------------------ the families
OVERFLOWING = ("cap_sizing", "cap_sizing_text", "cap_msgs_short1", "cap_fields_short1", "cap_sdps_short1",
               "cap_text_short1", "cap_spec_short1")
LONG_NAMES = ("call-id", "from", "to", "cseq", "via", "content-type", "content-length", "x" * 32)


def cases() -> list[Case]:
    out = [make("lines", lines()), make("content", content()), make("fuzz", fuzz(400, 7)),
           make("fuzz_all", fuzz(200, 8), fields=abi.HTTP_FIELDS_ALL)]
    pk, fl = ports()
    out.append(make("ports", pk, flags=fl))
    out.append(make("long_names", content(), names=LONG_NAMES, fields=abi.HTTP_FIELDS_ALL))
    # rules 2 and 3 for every combination of the flags they read, over a packet that is a message with KNOWN alone
    fc = flag_combinations()
    out.append(make("flags", [on_port(INVITE, k) for k in range(len(fc))], flags=fc))
    # hand-made records: rule 4
    p = on_port(INVITE, 1)
    n_, at = len(p), 42
    eth, ip4, udp = (1, 2, 0, 14, n_), (2, 3, 14, 20, n_ - 14), (sp.P_UDP, 4, 34, 8, n_ - 34)
    t = sp.packet(INVITE, 2, tcp=True)
    tcp = (sp.P_TCP, 4, 34, 20, len(t) - 34)
    teth, tip4 = (1, 2, 0, 14, len(t)), (2, 3, 14, 20, len(t) - 14)
    trailer = (sp.P_TRAILER, 2, n_ - 4, 4, 4)
    chains = [
        [eth, ip4, udp],                                           # as the parse writes it
        [eth, ip4, (sp.P_UDP, 4, 34, 8, n_ - 34 - 4), trailer],    # a trailer entry behind the carrier
        [eth, ip4, udp, trailer, trailer],                         # two entries behind it
        [eth, ip4, udp, (32, 7, at, n_ - at, n_ - at)],            # the carrier is not last: a Payload entry
        [eth, ip4, udp, (sp.P_TRAILER, 2, at, 4, 4), (32, 7, at, 4, 4)],
        [eth, ip4, (sp.P_UDP, 4, 34, 8, n_ - 34 + 1)],             # one byte past the packet
        [eth, ip4, (sp.P_UDP, 4, 35, 8, n_ - 34)],
        [eth, ip4, (sp.P_UDP, 4, 34, 8, 8)],                       # no payload: hdr_len == data_len
        [eth, ip4, (sp.P_UDP, 4, 34, n_ - 34 + 1, n_ - 34)],       # hdr_len > data_len
        [eth, ip4, (sp.P_UDP, 4, 34, 7, n_ - 34)],                 # hdr_len < 8
        [eth, ip4, (sp.P_UDP, 4, 34, 0, n_ - 34)],
        [eth, ip4, (sp.P_UDP, 4, 0xFFFF, 8, 100)],
        [eth, ip4, (sp.P_UDP, 4, 34, 8, 8 + 30)],                  # a shorter layer: the message cut at 30 bytes
        [eth, ip4, (sp.P_UDP, 4, 34, 8, 8 + 3)],                   # L = 3
        [(sp.P_UDP, 4, 34, 8, n_ - 34)],                           # the carrier as entry 0
        [eth, ip4, (sp.P_TCP, 4, 34, 8, n_ - 34)],                 # the UDP bytes recorded as TCP: the port path still
        [eth, (sp.P_UDP, 4, 14, 8, 40), ip4, udp],                 # two carriers: the last decides
        [eth, ip4, udp, (sp.P_UDP, 4, at, 8, 4)],                  # ... also when it is the bad one
        [eth, ip4],                                                # no carrier
        [eth, ip4, udp],                                           # n_layers 2: the carrier is not looked at
        [eth, ip4, udp],                                           # n_layers 9 > max_layers
        [eth, ip4, udp],                                           # n_layers 0
        [teth, tip4, tcp],                                         # TCP as the parse writes it
        [teth, tip4, (sp.P_TCP, 4, 34, 32, len(t) - 34)],          # options: the payload starts 12 bytes later
    ]
    nl = [None] * 19 + [2, 9, 0, None, None]
    pk = [p] * 22 + [t, t]
    out.append(make("records", pk, chains=chains, flags=[KNOWN] * len(pk), n_layers=nl))
    cut = make("cut_by_caplen", [on_port(INVITE, k) for k in range(6)], flags=[KNOWN] * 6)
    cut.caplens[1] -= 1           # the carrier's data_len reaches past caplen
    cut.caplens[2] = 42           # nothing of the payload
    cut.caplens[3] = 36           # inside the carrier's header
    cut.caplens[4] = 0
    out.append(cut)
    for ml in (1, 2, 3, 16):
        out.append(make(f"max_layers_{ml}", [sip_k(k) for k in range(1, 12)], ml=ml))
    # descriptors: the packets of a mixed batch with some descriptors out of bounds, the 64-bit wrap among them
    c = make("descriptors", mixed(40, "all"))
    c.offsets[5] = c.dlen() - 10
    c.offsets[11] = (1 << 64) - 20
    c.caplens[17] += 100000
    c.offsets[22] = c.dlen() + 1
    c.data_len = c.dlen() - 1
    c.offsets[30], c.caplens[30] = c.data_len, 0  # nothing at the very end: in bounds
    out.append(c)
    # the parse's own records
    out.append(parsed("parsed_mixed", mixed(200, "all") + lines()[::3] + content() + ports()[0][:len(PORTS) * 6]))
    out.append(parsed("parsed_ml2", mixed(64, "all"), abi.make_opts(max_layers=2)))
    # batch shapes around the wave and block edges
    for n in SIZES:
        for share in SHARES:
            out.append(make(f"n{n}_{share}", mixed(n, share)))
    out.append(make("n65_brief", mixed(65, "all"), use_brief=True))
    # every kinds / fields / text combination
    base = make("spec", mixed(70, "all") + lines()[::5] + content())
    for kinds in (1, 2, 3):
        for fields in (0, 1, 2):
            for text in (0, 1, 2, 3):
                out.append(replace(base, name=f"spec_k{kinds}_f{fields}_t{text}", kinds=kinds, fields=fields, text=text))
    out.append(replace(base, name="spec_no_names", names=()))
    out.append(replace(base, name="spec_8_names", names=LONG_NAMES))
    # capacities
    cap = make("cap_exact", mixed(130, "all"))
    m, k, nb, ns = needs(cap)
    out += [cap,
            replace(cap, name="cap_sizing", out_msgs=0, out_fields=0, out_sdps=0, text_cap=0, want_text=False,
                    want_disp=False),
            replace(cap, name="cap_sizing_text", out_msgs=0, out_fields=0, out_sdps=0, text_cap=0),
            replace(cap, name="cap_msgs_short1", out_msgs=m - 1),
            replace(cap, name="cap_fields_short1", out_fields=k - 1),
            replace(cap, name="cap_sdps_short1", out_sdps=ns - 1),
            replace(cap, name="cap_text_short1", text_cap=nb - 1),
            replace(cap, name="cap_spec_short1", max_msgs=m - 1),
            replace(cap, name="cap_spec_exact", max_msgs=m, out_msgs=m),
            replace(cap, name="cap_no_text", want_text=False, text_cap=0),
            replace(cap, name="cap_no_text_no_disp", want_text=False, want_disp=False, text_cap=0),
            replace(cap, name="cap_roomy", out_fields=k + 7, out_sdps=ns + 3, text_cap=nb + 100)]
    return out
