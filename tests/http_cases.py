"""Case generators and runners for pcppx_http_device / pcppx_http_reference (tests/test_http.py).

A Case is a source batch, its parse records (an input: written here the way the parse writes them -- an HTTP layer
behind Ethernet / IPv4 / TCP --, taken from the parse's restatement, or crafted), the spec and the output's capacities.
Three runners produce the same Buffers from it -- model() (pcapplusplus_amd.http.model, the contract in plain Python
over bytes.find), run_reference() (pcppx_http_reference) and run_device() (pcppx_http_device) -- every buffer pre-filled
with 0xA5 and over-allocated, so equality of the whole buffers also shows that nothing beyond the output was touched, and
nothing at all but the totals on overflow.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field, replace

import numpy as np

from pcapplusplus_amd import abi
from pcapplusplus_amd import http as ht
from pcapplusplus_amd.pcap import from_packets

BLOCK = 1024  # source packets per block of the kernels (pcppx_internal.h kHttpBlockPk)
ML = 6        # max_layers of the cases' records, unless a case says otherwise
FILL, F64 = 0xA5, 0xA5A5A5A5A5A5A5A5
PAD_BYTES, PAD_ENTRIES = 64, 4
ETH = abi.LINKTYPE_ETHERNET
AT = 54  # where the payload of ht.tcp_packet() starts
NONE, MSG, HOST, BAD = abi.HTTP_NONE, abi.HTTP_MSG, abi.HTTP_HOST, abi.HTTP_BAD_DESC
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
SHARES = (1, 100)  # per cent of HTTP packets
NAMES = ("host", "user-agent", "content-type", "content-length")


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

    def cap(self) -> int:
        return int(needs(self)[2]) if self.text_cap is None else self.text_cap


@dataclass
class Buffers:
    msgs: np.ndarray               # u8: (out_msgs + PAD_ENTRIES) * 48 bytes
    fields: np.ndarray             # u8: (out_fields + PAD_ENTRIES) * 24 bytes
    text: np.ndarray | None        # u8
    disposition: np.ndarray | None
    totals: np.ndarray

    def messages(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.HTTP_MSGS]) if k is None else k
        return self.msgs[:k * 48].view(abi.HTTP_MSG_DTYPE)

    def records(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.HTTP_FIELDS]) if k is None else k
        return self.fields[:k * 24].view(abi.HTTP_FIELD_DTYPE)

    def rows(self) -> list[tuple]:
        t = abi.http_totals_dict(self.totals)
        return ht.rows(self.messages(), self.records(), self.text[:t["text_bytes"]])


FIELDS = ("msgs", "fields", "text", "disposition")


def alloc(c: Case) -> Buffers:
    return Buffers(np.full((c.maxm() + PAD_ENTRIES) * 48, FILL, np.uint8),
                   np.full((c.maxf() + PAD_ENTRIES) * 24, FILL, np.uint8),
                   np.full(c.cap() + PAD_BYTES, FILL, np.uint8) if c.want_text else None,
                   np.full(c.n + PAD_ENTRIES, FILL, np.uint8) if c.want_disp else None,
                   np.full(abi.HTTP_TOTALS, F64, np.uint64))


# ------------------------------------------------------------------ runners
_MODEL: dict[tuple, tuple] = {}


def _result(c: Case, **kw) -> ht.Result:
    return ht.model(c.data, c.offsets, c.caplens, c.dlen(), c.summary["flags"], c.summary["n_layers"], c.layers, c.ml,
                    c.names, c.fields, c.text, c.kinds, **kw)


def needs(c: Case) -> tuple[int, int, int]:
    """(messages, records, text bytes) of the case's spec over its batch, whatever its capacities."""
    key = (id(c.data), id(c.offsets), id(c.caplens), id(c.layers), id(c.summary), c.ml, c.names, c.fields, c.text,
           c.kinds, c.data_len)
    if key not in _MODEL:
        r = _result(c)
        _MODEL[key] = (len(r.msgs), len(r.fields), len(r.text), c)  # c kept alive: the ids stay its own
    return _MODEL[key][:3]


def model(c: Case) -> Buffers:
    """include/pcppx.h's http contract, restated in pcapplusplus_amd/http.py, as the buffers a call leaves."""
    out = alloc(c)
    r = _result(c, max_msgs=c.max_msgs, out_msgs=c.maxm(), out_fields=c.maxf(), text_cap=c.cap(),
                want_text=c.want_text)
    out.totals[:] = r.totals
    if r.disposition is None:
        return out
    if out.disposition is not None:
        out.disposition[:c.n] = r.disposition
    out.msgs[:len(r.msgs) * 48] = ht.msgs_array(r.msgs).view(np.uint8)
    out.fields[:len(r.fields) * 24] = ht.fields_array(r.fields).view(np.uint8)
    if out.text is not None:
        out.text[:len(r.text)] = np.frombuffer(r.text, np.uint8)
    return out


def spec_of(c: Case) -> abi.HttpSpec:
    return abi.make_http_spec(c.names, c.fields, c.text, c.kinds, c.max_msgs)


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
    o = abi.HttpOut(out.msgs.ctypes.data, out.fields.ctypes.data, opt(out.text), c.cap(), opt(out.disposition),
                    c.maxm(), c.maxf(), out.totals.ctypes.data)
    abi.http_reference(b, r, c.ml, spec_of(c), o)
    del rec, lay
    return out


class DeviceRun:
    """A case's tensors on the device; launch() queues pcppx_http_device on a stream, result() reads the buffers."""

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
        self.d_msgs, self.d_fields = self.up(host.msgs), self.up(host.fields)
        self.d_text = None if host.text is None else self.up(host.text)
        self.d_disp = None if host.disposition is None else self.up(host.disposition)
        self.d_tot = self.up(host.totals.view(np.int64))

    def up(self, a: np.ndarray):
        import torch

        return torch.from_numpy(a).to(self.device)

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.http_device(self.data, self.offsets, self.caplens, c.n, ETH, self.layers, c.ml, spec_of(c), self.d_msgs,
                           self.d_fields, self.d_tot, c.maxm(), c.maxf(), self.d_text, c.cap(), self.d_disp, stream,
                           data_len=self.data_len, summary=self.summary, brief=self.brief)

    def result(self) -> Buffers:
        import torch

        torch.cuda.synchronize(self.device)
        down = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return Buffers(down(self.d_msgs), down(self.d_fields), down(self.d_text), down(self.d_disp),
                       down(self.d_tot).view(np.uint64))


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
    """The all-or-nothing rule: the messages, the records, the text and the dispositions still hold the fill."""
    for f in FIELDS:
        g = getattr(got, f)
        assert g is None or bool((g == FILL).all()), (what, f)


# ------------------------------------------------------------------ records
def chain_of(pkt: bytes) -> list[tuple]:
    """The chain the parse records for a packet of ht.tcp_packet(): (proto, osi, offset, hdr_len, data_len) per layer.
    A payload on port 80 is an HTTP layer -- a response when it starts with "HTTP", else a request -- whose header is
    what the model's walk measures, with the rest as a generic payload layer (proto 0x20 here) behind it."""
    chain = [(1, 2, 0, 14, len(pkt)), (2, 3, 14, 20, len(pkt) - 14), (4, 4, 34, 20, len(pkt) - 34)]
    left = len(pkt) - AT
    ports = (int.from_bytes(pkt[34:36], "big"), int.from_bytes(pkt[36:38], "big"))
    if left > 0 and 80 in ports:
        kind = 1 if pkt[AT:AT + 4] == b"HTTP" else 0
        hdr = ht.message(0, AT, kind, pkt[AT:]).header_len
        chain.append((ht.P_REQUEST + kind, 7, AT, hdr, left))
        if hdr < left:
            chain.append((32, 7, AT + hdr, left - hdr, left - hdr))
    elif left > 0:
        chain.append((32, 7, AT, left, left))
    return chain


def make(name: str, packets: list[bytes], chains: list | None = None, flags: list | None = None, ml: int = ML,
         n_layers: list | None = None, **kw) -> Case:
    """A case over the packets back to back. chains[i]: packet i's layer entries (None: chain_of it), of which the
    first ml are recorded; n_layers[i] (None: the chain's length capped at ml, as the parse caps it)."""
    n = len(packets)
    caps = np.array([len(p) for p in packets], np.uint32)
    offs = (np.cumsum(caps, dtype=np.uint64) - caps).astype(np.uint64)
    data = np.frombuffer(b"".join(packets) + b"\0", np.uint8).copy()
    summary = np.zeros(n, abi.SUMMARY_DTYPE)
    layers = np.zeros((n, ml), abi.LAYER_DTYPE)
    for i, p in enumerate(packets):
        chain = chain_of(p) if chains is None or chains[i] is None else chains[i]
        for k, e in enumerate(chain[:ml]):
            layers[i, k] = e
        summary["n_layers"][i] = min(len(chain), ml) if n_layers is None or n_layers[i] is None else n_layers[i]
        over = abi.F_DEPTH_OVERFLOW if len(chain) > ml else 0
        summary["flags"][i] = over if flags is None or flags[i] is None else flags[i]
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
def req(payload: bytes, k: int = 0) -> bytes:
    return ht.tcp_packet(payload, k, False)


def res(payload: bytes, k: int = 0) -> bytes:
    return ht.tcp_packet(payload, k, True)


GET = b"GET /index.html HTTP/1.1\r\n"
OK = b"HTTP/1.1 200 OK\r\n"

# rule 4, one branch a line: (name, payload)
REQUEST_LINES = [
    ("get", GET + b"Host: a\r\n\r\n"),
    ("L_below_4", b"GET"),
    ("L_4_no_space", b"GETX"),
    ("space_at_0", b" GET / HTTP/1.1\r\n\r\n"),
    ("no_space", b"GET/index.htmlHTTP/1.1"),
    ("space_at_last_byte", b"OPTIONS "),
    ("unknown_method", b"BREW /pot HTTP/1.1\r\nHost: a\r\n\r\n"),
    ("lower_case_method", b"get / HTTP/1.1\r\n\r\n"),
    ("method_of_8_bytes", b"OPTIONSX / HTTP/1.1\r\n\r\n"),
    ("no_version", b"GET /index.html\r\nHost: a\r\n\r\n"),
    ("version_cut_v_plus_8", b"GET / HTTP/1."),
    ("version_at_v_plus_9", b"GET / HTTP/1.1"),
    ("version_unknown_text", b"GET / HTTP/2.0\r\nHost: a\r\n\r\n"),
    ("version_0_9", b"GET / HTTP/0.9\r\n\r\n"),
    ("version_1_0", b"POST /p HTTP/1.0\r\nContent-Length: 3\r\n\r\nabc"),
    ("version_no_dot", b"GET / HTTP/1x1\r\n\r\n"),
    ("no_newline", b"GET /a/b/c HTTP/1.1 and then nothing"),
    ("empty_uri", b"GET  HTTP/1.1\r\n\r\n"),
    ("uri_with_spaces", b"GET /a b c HTTP/1.1\r\n\r\n"),
    ("two_versions", b"GET /x HTTP/1.0 HTTP/1.1\r\n\r\n"),
    ("space_http_in_header", b"GET /x\r\nX: y HTTP/1.1\r\n\r\n"),
    ("lf_only", b"GET / HTTP/1.1\nHost: a\n\n"),
    ("almost_version", b"GET / HTTP HTTP/ HTTP/1.1\r\n\r\n"),
]
METHOD_LINES = [(f"method_{m}", f"{m} /m HTTP/1.1\r\nHost: m\r\n\r\n".encode()) for m in abi.HTTP_METHODS]

# rule 5
RESPONSE_LINES = [
    ("ok", OK + b"Content-Length: 0\r\n\r\n"),
    ("L_below_8", b"HTTP/1."),
    ("L_8", b"HTTP/1.1"),
    ("not_http", b"HTTQ/1.1 200 OK\r\n\r\n"),
    ("version_unknown", b"HTTP/3.0 200 OK\r\n\r\n"),
    ("version_1_0", b"HTTP/1.0 404 Not Found\r\n\r\n"),
    ("version_0_9", b"HTTP/0.9 200 OK\r\n\r\n"),
    ("L_11", b"HTTP/1.1 20"),
    ("L_12", b"HTTP/1.1 200"),
    ("L_13", b"HTTP/1.1 200 "),
    ("L_14_lf", b"HTTP/1.1 200 \n"),
    ("no_newline", b"HTTP/1.1 200 OK"),
    ("code_not_digits", b"HTTP/1.1 2x0 OK\r\n\r\n"),
    ("code_space", b"HTTP/1.1  20 OK\r\n\r\n"),
    ("empty_message_crlf", b"HTTP/1.1 200 \r\n\r\n"),
    ("empty_message_lf", b"HTTP/1.1 200 \nA: b\n\n"),
    ("message_cr_only", b"HTTP/1.1 200 \r\r\n\r\n"),
    ("message_lf", b"HTTP/1.1 301 Moved Permanently\nLocation: /x\n\n"),
    ("newline_before_13", b"HTTP/1.1 200\nOK and more\nA: b\n\n"),
    ("code_599", b"HTTP/1.1 599 Custom thing\r\n\r\n"),
    ("code_099", b"HTTP/1.1 099 Low\r\n\r\n"),
    ("no_space_before_message", b"HTTP/1.1 200OK\r\n\r\n"),
]

# rules 6-8: the header behind a complete first line
FIELD_CASES = [
    ("plain", b"Host: example.com\r\nUser-Agent: x/1.0\r\nAccept: */*\r\n\r\n"),
    ("first_line_len_is_L", b""),
    ("end_at_once_crlf", b"\r\n"),
    ("end_at_once_lf", b"\n"),
    ("end_at_once_cr", b"\rxyz"),
    ("lf_lf", b"A: b\n\n"),
    ("crlf_crlf", b"A: b\r\n\r\n"),
    ("line_starts_with_colon", b": value\r\nHost: a\r\n\r\n"),
    ("colon_only_line_last", b"Host: a\r\n:"),
    ("colon_behind_nul", b"Na\0me: value-behind-nul"),
    ("nul_then_more", b"A: b\r\nXY\0Z: 1\r\n\r\n"),
    ("nul_at_field_start", b"A: b\r\n\0rest: 1"),
    ("name_colon_at_last_byte", b"Host: a\r\nName:"),
    ("spaces_to_the_end", b"Host: a\r\nName:     "),
    ("spaces_then_newline", b"Name:   \r\nHost: a\r\n\r\n"),
    ("value_empty_crlf", b"Name:\r\nHost:\n\r\n"),
    ("no_colon_line", b"no colon here\r\nHost: a\r\n\r\n"),
    ("colon_on_a_later_line", b"first line without\r\nsecond: has\r\n\r\n"),
    ("colon_at_e", b"abc\n:def\n\n"),
    ("no_newline_with_value", b"Host: cut.example"),
    ("no_newline_no_colon", b"Hostcut"),
    ("value_cr_inside", b"A: b\rc\r\n\r\n"),
    ("value_ends_cr_cr", b"A: b\r\r\n\r\n"),
    ("many_spaces", b"A:      b  \r\n\r\n"),
    ("tab_is_value", b"A:\tb\r\n\r\n"),
    ("header_incomplete", b"Host: a\r\nUser-Agent: b\r\n"),
    ("header_incomplete_cut", b"Host: a\r\nUser-Age"),
    ("empty_name_last", b"Host: a\r\n: x"),
    ("repeated_host", b"Host: one\r\nhost: two\r\nHOST: three\r\nX: y\r\n\r\n"),
    ("name_trailing_space", b"Host : a\r\nHost: b\r\n\r\n"),
    ("upper_lower", b"HOST: A\r\nUsEr-AgEnT: B\r\ncontent-TYPE: text/html; charset=x\r\n\r\n"),
    ("name_32_bytes", b"abcdefghijklmnopqrstuvwxyz012345: v\r\nabcdefghijklmnopqrstuvwxyz0123456: w\r\n\r\n"),
    ("name_non_ascii", b"H\xd6ST: a\r\nhost\x00: b\r\n\r\n"),
    ("body_behind", b"Host: a\r\n\r\nHost: in-the-body\r\n\r\n"),
    ("linear", b"x" * 3 + b"\r\n" + b"".join(b"l%d\r\n" % j for j in range(700)) + b"last: one\r\n\r\n"),
]

CONTENT_LENGTHS = [b"", b" +12x", b"-5", b"2147483647", b"2147483648", b"123456789012345678901234567890", b"0",
                   b"42", b"\t\v\f\r 7", b"+", b"-", b"- 5", b"12\x0034", b"0000000000000000000012", b"-2147483648",
                   b"4294967296", b"9x", b"x9"]
LONG_NAMES = ("host ", "host", "abcdefghijklmnopqrstuvwxyz012345", "x-forwarded-for", "content-length", ":", "h\xd6st",
              "a")


def lines() -> list[bytes]:
    out = [req(p, k) for k, (_, p) in enumerate(REQUEST_LINES)]
    out += [req(p, k) for k, (_, p) in enumerate(METHOD_LINES)]
    out += [res(p, k) for k, (_, p) in enumerate(RESPONSE_LINES)]
    return out


def header_cases() -> list[bytes]:
    out = []
    for k, (_, h) in enumerate(FIELD_CASES):
        out.append(req(GET + h, k))
        out.append(res(OK + h, k))
    return out


def content_lengths() -> list[bytes]:
    out = []
    for k, v in enumerate(CONTENT_LENGTHS):
        out.append(res(OK + b"Content-Length: " + v + b"\r\nX: y\r\n\r\n", k))
        out.append(req(b"POST /u HTTP/1.1\r\ncontent-LENGTH:" + v + b"\r\nContent-Length: 99\r\n\r\n", k))
    out.append(res(OK + b"Content-Length", 1))                    # no colon, no line end: the line is the name
    out.append(res(OK + b"Content-Length:", 2))                   # no value: atoi("")
    out.append(res(OK + b"Content-Length: 77", 3))                # no line end
    out.append(res(OK + b"X-Content-Length: 5\r\nContent-Length : 6\r\n\r\n", 4))  # neither is the name
    out.append(res(b"HTTP/1.1 200 OK\r\n\r\nContent-Length: 5\r\n\r\n", 5))         # behind the header's end
    return out


AGENTS = ("Mozilla/5.0 (X11; Linux x86_64)", "curl/8.0", "Wget/1.21")
TYPES = ("text/html; charset=utf-8", "application/json", "image/png", "text/css;q=1")


def http_k(k: int) -> bytes:
    """HTTP packet k of the mixed batches: requests and responses in turn, a few incomplete or odd."""
    if k % 2 == 0:
        h = [("Host", f"h{k % 97}.example.org"), ("User-Agent", AGENTS[k % 3]), ("Accept", "*/*")]
        h += [("Cookie", "c=" + "z" * (k % 211))] if k % 5 == 0 else []
        body = b""
        if k % 7 == 0:
            body = b"b" * (k % 50)
            h += [("Content-Type", "application/x-www-form-urlencoded"), ("Content-Length", str(len(body)))]
        p = ht.request(abi.HTTP_METHODS[k % 9] if k % 7 else "POST", f"/p/{k}?q={k % 13}", h, body=body,
                       end=k % 17 != 0)
        return req(p[:len(p) - (k % 29 if k % 23 == 0 else 0)], k)
    h = [("Server", "srv"), ("Content-Type", TYPES[k % 4]), ("Content-Length", str(k % 1000))]
    h += [("Set-Cookie", "s=" + "y" * (k % 97))] if k % 3 == 0 else []
    code, msg = ((200, "OK"), (404, "Not Found"), (304, "Not Modified"), (500, "Internal Server Error"))[k % 4]
    return res(ht.response(code, msg, h, body=bytes(j % 251 for j in range(k % 120)),
                           eol=b"\n" if k % 11 == 0 else b"\r\n"), k)


def other_k(k: int) -> bytes:
    """A packet without an HTTP layer: a TCP ACK or a payload on another port."""
    if k % 2:
        return ht.tcp_packet(b"", k, port=443)
    return ht.tcp_packet(bytes(1 + (k + j) % 250 for j in range(20 + k % 30)), k, port=4000 + k % 10)


def mixed(n: int, share: int) -> list[bytes]:
    """n packets with `share` per cent HTTP; the heaviest header of the cases sits at the first and at the last lane of
    a tile."""
    step = {0: 0, 1: 97, 100: 1}[share]
    out = [http_k(k) if step and k % step == 0 else other_k(k) for k in range(n)]
    heavy = req(GET + FIELD_CASES[-1][1], 7)
    out[0] = heavy
    if n >= 128:
        out[(n // 64 - 1) * 64 + 63] = heavy
    return out


FLAG_BITS = (abi.F_NEEDS_HOST_L7, abi.F_NEEDS_HOST_PROTO, abi.F_DEPTH_OVERFLOW, abi.F_OVERSIZE, abi.F_BAD_DESC,
             abi.F_L7_KNOWN, abi.F_L7_SSL, abi.F_L7_HTTP)


def flag_combinations() -> list[int]:
    return [sum(b for j, b in enumerate(FLAG_BITS) if (m >> j) & 1) | (abi.F_IP_CSUM if m % 3 == 0 else 0)
            for m in range(256)]


MUTATION_BYTES = (0x00, 0x0A, 0x0D, 0x20, 0x3A, 0x09, 0x41, 0x7A, 0xFF)


def mutate(m: bytearray, rng, first: int = 0) -> None:
    """One to four seeded changes to the HTTP message that starts at m[first]: a random byte, one of the bytes the
    rules look for, a bit flip, or a swap of two bytes."""
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
    """Seeded mutations of the crafted messages, a third of them cut short."""
    rng = np.random.default_rng(seed)
    base = [p for _, p in REQUEST_LINES] + [p for _, p in METHOD_LINES] + [p for _, p in RESPONSE_LINES] + \
        [GET + h for _, h in FIELD_CASES[:-1]] + [OK + h for _, h in FIELD_CASES[:-1]]
    out = []
    for k in range(count):
        m = bytearray(base[int(rng.integers(len(base)))])
        mutate(m, rng)
        if len(m) > 1 and rng.integers(3) == 0:
            m = m[:int(rng.integers(1, len(m) + 1))]
        out.append(res(bytes(m), k) if m[:4] == b"HTTP" else req(bytes(m), k))
    return out


# ------------------------------------------------------------------ the frozen answers of the real HTTP layers
# tests/golden/http/fields.npz (tools/make_golden_http.py writes it, the tests read it): one JSON text per file, a list
# with one entry per packet: null where the reference builds no HTTP layer, else
#   [kind, getHeaderLen(), getFieldCount(), isHeaderComplete(), the first line's getSize(), method, version, URI or
#    status message as hex, getStatusCodeAsInt(), the first line's isComplete(), content length, has a content-length
#    field, [[name as hex, value as hex, getFieldSize(), isEndOfHeader(), getFieldByName(name) is this field], ...]]
def save_frozen(path, frozen: dict) -> None:
    files = sorted(frozen)
    np.savez_compressed(path, files=np.array(files),
                        **{f"f{k}": np.frombuffer(json.dumps(frozen[f], separators=(",", ":")).encode(), np.uint8)
                           for k, f in enumerate(files)})


def load_frozen(path) -> dict:
    z = np.load(path, allow_pickle=False)
    return {str(f): json.loads(z[f"f{k}"].tobytes().decode()) for k, f in enumerate(z["files"])}


# ------------------------------------------------------------------ the families
OVERFLOWING = ("cap_sizing", "cap_sizing_text", "cap_msgs_short1", "cap_fields_short1", "cap_text_short1",
               "cap_spec_short1")


def cases() -> list[Case]:
    out = [make("lines", lines()), make("headers", header_cases()), make("content_length", content_lengths()),
           make("fuzz", fuzz(400, 7)), make("fuzz_all", fuzz(200, 8), fields=abi.HTTP_FIELDS_ALL)]
    out.append(make("long_names", header_cases(), names=LONG_NAMES, fields=abi.HTTP_FIELDS_ALL))
    # rule 3 for every combination of the flags it reads, without and with a recorded HTTP layer
    fl = flag_combinations()
    out.append(make("flags", [other_k(2 * k) for k in range(256)] + [http_k(1), http_k(2)], flags=fl + [0xFFFF, fl[37]]))
    # hand-made records: a layer the parse would not record (an unknown method, a bad status code), the layer outside the
    # packet, n_layers against max_layers, HTTP as entry 0, two HTTP entries, the kind against the bytes
    p = req(ht.request("GET", "/r", [("Host", "rec")], body=b"body"), 1)
    n_, at = len(p), AT
    eth, ip4, tcp = (1, 2, 0, 14, n_), (2, 3, 14, 20, n_ - 14), (4, 4, 34, 20, n_ - 34)
    h = lambda proto, o, hl, dl: (proto, 7, o, hl, dl)  # noqa: E731
    bad_method, bad_code = req(b"BREW / HTTP/1.1\r\nHost: x\r\n\r\n", 2), res(b"HTTP/1.1 abc Nope\r\nA: b\r\n\r\n", 3)
    chains = [
        [eth, ip4, tcp, h(6, at, n_ - at - 4, n_ - at)],        # as the parse writes it
        [eth, ip4, tcp, h(6, at, n_ - at, n_ - at + 1)],        # one byte past the packet
        [eth, ip4, tcp, h(6, at + 1, n_ - at, n_ - at)],
        [eth, ip4, tcp, h(6, at, n_ - at + 1, n_ - at)],        # hdr_len > data_len
        [eth, ip4, tcp, h(6, 0xFFFF, 12, 12)],
        [eth, ip4, tcp, h(6, at, 3, 3)],                        # a shorter layer: L = 3
        [eth, ip4, tcp, h(6, at, 0, 0)],                        # L = 0
        [eth, ip4, tcp, h(6, n_, 0, 0)],                        # L = 0 at the packet's end
        [eth, ip4, tcp, h(7, at, n_ - at, n_ - at)],            # a request's bytes recorded as a response
        [h(6, at, n_ - at, n_ - at)],                           # HTTP as entry 0
        [eth, ip4, tcp, h(6, at, n_ - at, n_ - at + 9), h(6, at, n_ - at, n_ - at)],  # the first HTTP entry decides
        [eth, ip4, tcp, (32, 7, at, 4, 4), h(6, at, n_ - at, n_ - at)],
        [eth, ip4, tcp, h(6, at, n_ - at, n_ - at)],            # n_layers 3: the entry is not looked at
        [eth, ip4, tcp, h(6, at, n_ - at, n_ - at)],            # n_layers 9 > max_layers
        [eth, ip4, tcp],                                        # n_layers 9 > max_layers, no HTTP entry: HOST
        [eth, ip4, tcp, h(6, at, n_ - at, n_ - at)],            # n_layers 0
        [eth, ip4, tcp, h(6, at, n_ - at - 7, n_ - at - 7)],    # cut inside the header
    ]
    nl = [None] * 12 + [3, 9, 9, 0, None]
    pk = [p] * len(chains) + [bad_method, bad_code]
    lb, lc = len(bad_method), len(bad_code)
    chains += [[(1, 2, 0, 14, lb), (2, 3, 14, 20, lb - 14), (4, 4, 34, 20, lb - 34), h(6, at, lb - at, lb - at)],
               [(1, 2, 0, 14, lc), (2, 3, 14, 20, lc - 14), (4, 4, 34, 20, lc - 34), h(7, at, lc - at, lc - at)]]
    out.append(make("records", pk, chains=chains, n_layers=nl + [None, None]))
    for ml in (1, 3, 4, 16):
        out.append(make(f"max_layers_{ml}", [http_k(k) for k in range(1, 12)], ml=ml))
    # descriptors: the packets of a mixed batch with some descriptors out of bounds, the 64-bit wrap among them
    c = make("descriptors", mixed(40, 100))
    c.offsets[5] = c.dlen() - 10
    c.offsets[11] = (1 << 64) - 20
    c.caplens[17] += 100000
    c.offsets[22] = c.dlen() + 1
    c.data_len = c.dlen() - 1
    c.offsets[30], c.caplens[30] = c.data_len, 0  # nothing at the very end: in bounds
    out.append(c)
    # the parse's own records
    out.append(parsed("parsed_mixed", mixed(200, 100) + lines() + header_cases()[:40]))
    out.append(parsed("parsed_ml3", mixed(64, 100), abi.make_opts(max_layers=3)))
    # batch shapes around the wave and block edges
    for n in SIZES:
        for share in SHARES:
            out.append(make(f"n{n}_s{share}", mixed(n, share)))
    out.append(make("n0", []))
    out.append(make("n65_brief", mixed(65, 100), use_brief=True))
    # every kinds / fields / text combination
    base = make("spec", mixed(70, 100) + lines() + header_cases())
    for kinds in (1, 2, 3):
        for fields in (0, 1, 2):
            for text in (0, 1, 2, 3):
                out.append(replace(base, name=f"spec_k{kinds}_f{fields}_t{text}", kinds=kinds, fields=fields, text=text))
    out.append(replace(base, name="spec_no_names", names=()))
    out.append(replace(base, name="spec_8_names", names=LONG_NAMES, fields=abi.HTTP_FIELDS_WANTED))
    # capacities
    cap = make("cap_exact", mixed(130, 100))
    m, k, nb = needs(cap)
    out += [cap,
            replace(cap, name="cap_sizing", out_msgs=0, out_fields=0, text_cap=0, want_text=False, want_disp=False),
            replace(cap, name="cap_sizing_text", out_msgs=0, out_fields=0, text_cap=0),
            replace(cap, name="cap_msgs_short1", out_msgs=m - 1),
            replace(cap, name="cap_fields_short1", out_fields=k - 1),
            replace(cap, name="cap_text_short1", text_cap=nb - 1),
            replace(cap, name="cap_spec_short1", max_msgs=m - 1),
            replace(cap, name="cap_spec_exact", max_msgs=m, out_msgs=m),
            replace(cap, name="cap_no_text", want_text=False, text_cap=0),
            replace(cap, name="cap_no_text_no_disp", want_text=False, want_disp=False, text_cap=0),
            replace(cap, name="cap_roomy", out_fields=k + 7, text_cap=nb + 100)]
    return out
