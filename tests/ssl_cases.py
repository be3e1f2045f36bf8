"""Case generators and runners for pcppx_ssl_device / pcppx_ssl_reference (tests/test_ssl.py).

A Case is a source batch, its parse records (an input: written here the way the parse writes them -- one SSL entry per
TLS record behind Ethernet / IPv4 / TCP --, taken from the parse's restatement, or crafted), the spec and the output's
capacities. Three runners produce the same Buffers from it -- model() (pcapplusplus_amd.ssl.model, the contract in plain
Python over byte slices), run_reference() (pcppx_ssl_reference) and run_device() (pcppx_ssl_device) -- every buffer
pre-filled with 0xA5 and over-allocated, so equality of the whole buffers also shows that nothing beyond the output was
touched, and nothing at all but the totals on overflow.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

from pcapplusplus_amd import abi
from pcapplusplus_amd import ssl as sl
from pcapplusplus_amd.pcap import from_packets

BLOCK = 1024  # source packets per block of the kernels (pcppx_internal.h kSslBlockPk)
ML = 8        # max_layers of the cases' records, unless a case says otherwise
FILL, F64 = 0xA5, 0xA5A5A5A5A5A5A5A5
PAD_BYTES, PAD_ENTRIES = 64, 4
ETH = abi.LINKTYPE_ETHERNET
AT = 54  # where the payload of sl.tcp_packet() starts
NONE, MSG, HOST, BAD = abi.SSL_NONE, abi.SSL_MSG, abi.SSL_HOST, abi.SSL_BAD_DESC
SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)
SHARES = (1, 100)  # per cent of SSL packets


@dataclass
class Case:
    name: str
    data: np.ndarray      # u8
    offsets: np.ndarray   # u64
    caplens: np.ndarray   # u32
    summary: np.ndarray   # SUMMARY_DTYPE[n]: flags and n_layers are read
    layers: np.ndarray    # LAYER_DTYPE[n, ml]
    ml: int = ML
    kinds: int = 3
    max_msgs: int = 0               # the spec's
    out_msgs: int | None = None     # None: n
    out_hellos: int | None = None   # None: exactly what the records need
    names_cap: int | None = None    # None: exactly what the names need
    want_names: bool = True
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

    def maxh(self) -> int:
        return int(needs(self)[1]) if self.out_hellos is None else self.out_hellos

    def cap(self) -> int:
        return int(needs(self)[2]) if self.names_cap is None else self.names_cap


@dataclass
class Buffers:
    msgs: np.ndarray               # u8: (out_msgs + PAD_ENTRIES) * 32 bytes
    hellos: np.ndarray             # u8: (out_hellos + PAD_ENTRIES) * 32 bytes
    names: np.ndarray | None       # u8
    disposition: np.ndarray | None
    totals: np.ndarray

    def messages(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.SSL_MSGS]) if k is None else k
        return self.msgs[:k * 32].view(abi.SSL_MSG_DTYPE)

    def records(self, k: int | None = None) -> np.ndarray:
        k = int(self.totals[abi.SSL_HELLOS]) if k is None else k
        return self.hellos[:k * 32].view(abi.SSL_HELLO_DTYPE)

    def name_bytes(self) -> bytes:
        return b"" if self.names is None else self.names[:int(self.totals[abi.SSL_NAME_BYTES])].tobytes()

    def rows(self) -> list[tuple]:
        return sl.rows(self.messages(), self.records(), self.name_bytes())


FIELDS = ("msgs", "hellos", "names", "disposition")


def alloc(c: Case) -> Buffers:
    return Buffers(np.full((c.maxm() + PAD_ENTRIES) * 32, FILL, np.uint8),
                   np.full((c.maxh() + PAD_ENTRIES) * 32, FILL, np.uint8),
                   np.full(c.cap() + PAD_BYTES, FILL, np.uint8) if c.want_names else None,
                   np.full(c.n + PAD_ENTRIES, FILL, np.uint8) if c.want_disp else None,
                   np.full(abi.SSL_TOTALS, F64, np.uint64))


# ------------------------------------------------------------------ runners
_MODEL: dict[tuple, tuple] = {}


def _result(c: Case, **kw) -> sl.Result:
    return sl.model(c.data, c.offsets, c.caplens, c.dlen(), c.summary["flags"], c.summary["n_layers"], c.layers, c.ml,
                    c.kinds, **kw)


def needs(c: Case) -> tuple[int, int, int]:
    """(messages, hello records, name bytes) of the case's spec over its batch, whatever its capacities."""
    key = (id(c.data), id(c.offsets), id(c.caplens), id(c.layers), id(c.summary), c.ml, c.kinds, c.data_len)
    if key not in _MODEL:
        r = _result(c)
        _MODEL[key] = (len(r.msgs), len(r.hellos), len(r.names), c)  # c kept alive: the ids stay its own
    return _MODEL[key][:3]


def model(c: Case) -> Buffers:
    """include/pcppx.h's ssl contract, restated in pcapplusplus_amd/ssl.py, as the buffers a call leaves."""
    out = alloc(c)
    r = _result(c, max_msgs=c.max_msgs, out_msgs=c.maxm(), out_hellos=c.maxh(), names_cap=c.cap(),
                want_names=c.want_names)
    out.totals[:] = r.totals
    if r.disposition is None:
        return out
    if out.disposition is not None:
        out.disposition[:c.n] = r.disposition
    out.msgs[:len(r.msgs) * 32] = sl.msgs_array(r.msgs).view(np.uint8)
    out.hellos[:len(r.hellos) * 32] = sl.hellos_array(r.hellos).view(np.uint8)
    if out.names is not None:
        out.names[:len(r.names)] = np.frombuffer(r.names, np.uint8)
    return out


def spec_of(c: Case) -> abi.SslSpec:
    return abi.make_ssl_spec(c.kinds, c.max_msgs)


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
    o = abi.SslOut(out.msgs.ctypes.data, out.hellos.ctypes.data, opt(out.names), c.cap(), opt(out.disposition),
                   c.maxm(), c.maxh(), out.totals.ctypes.data)
    abi.ssl_reference(b, r, c.ml, spec_of(c), o)
    del rec, lay
    return out


class DeviceRun:
    """A case's tensors on the device; launch() queues pcppx_ssl_device on a stream, result() reads the buffers."""

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
        self.d_msgs, self.d_hellos = self.up(host.msgs), self.up(host.hellos)
        self.d_names = None if host.names is None else self.up(host.names)
        self.d_disp = None if host.disposition is None else self.up(host.disposition)
        self.d_tot = self.up(host.totals.view(np.int64))

    def up(self, a: np.ndarray):
        import torch

        return torch.from_numpy(a).to(self.device)

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.ssl_device(self.data, self.offsets, self.caplens, c.n, ETH, self.layers, c.ml, spec_of(c), self.d_msgs,
                          self.d_hellos, self.d_tot, c.maxm(), c.maxh(), self.d_names, c.cap(), self.d_disp, stream,
                          data_len=self.data_len, summary=self.summary, brief=self.brief)

    def result(self) -> Buffers:
        import torch

        torch.cuda.synchronize(self.device)
        down = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return Buffers(down(self.d_msgs), down(self.d_hellos), down(self.d_names), down(self.d_disp),
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
    """The all-or-nothing rule: the messages, the records, the names and the dispositions still hold the fill."""
    for f in FIELDS:
        g = getattr(got, f)
        assert g is None or bool((g == FILL).all()), (what, f)


# ------------------------------------------------------------------ records
def chain_of(pkt: bytes) -> list[tuple]:
    """The chain the parse records for a packet of sl.tcp_packet(): (proto, osi, offset, hdr_len, data_len) per layer.
    A payload on an SSL port that starts with a record type is one SSL entry per TLS record: hdr_len = 5 + the
    record's length cut at the rest of the packet, data_len = the rest; the next entry follows while a record header
    with a known type is left."""
    chain = [(1, 2, 0, 14, len(pkt)), (2, 3, 14, 20, len(pkt) - 14), (4, 4, 34, 20, len(pkt) - 34)]
    ports = (int.from_bytes(pkt[34:36], "big"), int.from_bytes(pkt[36:38], "big"))
    ro, rem = AT, len(pkt) - AT
    if not any(p in sl.SSL_PORTS for p in ports) or rem < 5 or not 20 <= pkt[ro] <= 23:
        return chain + ([(32, 7, ro, rem, rem)] if rem > 0 else [])
    while True:
        hl = min(5 + int.from_bytes(pkt[ro + 3:ro + 5], "big"), rem)
        chain.append((sl.P_SSL, 6, ro, hl, rem))
        if rem - hl < 5 or not 20 <= pkt[ro + hl] <= 23:
            return chain
        ro, rem = ro + hl, rem - hl


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
def cli(payload: bytes, k: int = 0, port: int = 443) -> bytes:
    return sl.tcp_packet(payload, k, False, port)


def srv(payload: bytes, k: int = 0, port: int = 443) -> bytes:
    return sl.tcp_packet(payload, k, True, port)


HS, CCS, ALERT, APP = sl.HANDSHAKE, sl.CCS, sl.ALERT, sl.APPDATA
R = sl.record
GROUPS = sl.extension(10, b"\x00\x04\x00\x1d\x00\x17")
ALPN = sl.extension(16, b"\x00\x03\x02h2")
CH = sl.client_hello([sl.sni(b"www.example.org"), GROUPS, ALPN])
SH = sl.server_hello([sl.extension(0xFF01, b"\x00")])
SH13 = sl.server_hello([sl.extension(43, b"\x03\x04"), sl.extension(51, bytes(36))], cipher=0x1301, sid=bytes(32))
CERT = sl.handshake(11, bytes(j % 251 for j in range(300)))
DONE = sl.handshake(14, b"")
ENC = bytes((7 * j + 3) % 256 for j in range(40))  # an encrypted handshake message: byte 1 is not 0

# rule 3: (name, payload) -- each record type alone and mixed
RECORD_TYPES = [
    ("ccs", R(CCS, b"\x01")),
    ("alert", R(ALERT, b"\x02\x28")),
    ("handshake_client", R(HS, CH)),
    ("handshake_server", R(HS, SH)),
    ("appdata", R(APP, bytes(100))),
    ("server_flight", R(HS, SH) + R(HS, CERT) + R(HS, DONE)),
    ("client_finish", R(HS, sl.handshake(16, bytes(66))) + R(CCS, b"\x01") + R(HS, ENC)),
    ("app_then_alert", R(APP, bytes(30)) + R(ALERT, b"\x01\x00")),
    ("all_four", R(HS, CH) + R(CCS, b"\x01") + R(ALERT, b"\x01\x00") + R(APP, bytes(9)) + R(APP, bytes(5))),
    ("record_cut", R(APP, bytes(10), length=500)),
    ("empty_record", R(APP, b"")),
    ("ssl3_hello", R(HS, sl.client_hello(None, version=0x0300), version=0x0300)),
]

# rules 4-7: (name, the body of one handshake record)
HELLOS = [
    ("client_plain", CH),
    ("server_plain", SH),
    ("server_tls13", SH13),
    ("both_client_first", CH + SH),
    ("both_server_first", SH + CH),
    ("two_clients", sl.client_hello([sl.sni(b"first")]) + sl.client_hello([sl.sni(b"second")])),
    ("behind_type_8", sl.handshake(8, b"\x00\x00") + CH),        # EncryptedExtensions: not in the switch
    ("behind_type_22", sl.handshake(22, b"\x00") + SH),
    ("behind_type_3", sl.handshake(3, b"") + CH),
    ("behind_type_255", sl.handshake(255, b"") + CH),
    ("behind_hello_request", sl.handshake(0, b"") + CH),
    ("behind_certificate", CERT + SH + DONE),
    ("behind_finished", sl.handshake(20, bytes(12)) + CH),
    ("five_zeros_D15", bytes(8) + sl.handshake(1, b"\x03\x03\x09")),   # 4 + 4 + a ClientHello of 7 bytes
    ("five_zeros_D16", bytes(8) + sl.handshake(1, b"\x03\x03\x09\x09")),
    ("byte1_D15", sl.handshake(1, b"\x03\x01" + bytes(9), length1=1)),
    ("byte1_D16", sl.handshake(1, b"\x03\x01" + bytes(10), length1=1)),
    ("byte1_behind", DONE + sl.handshake(1, CH[4:], length1=2)),
    ("D_3", b"\x01\x00\x00"),
    ("D_4", sl.handshake(1, b"")),
    ("D_5", sl.handshake(2, b"\x03")),
    ("D_6", sl.handshake(2, b"\x03\x02")),
    ("M_beyond_D", sl.client_hello([sl.sni(b"cut.example")], length=5000)),
    ("M_cuts_extensions", sl.client_hello([GROUPS, sl.sni(b"lost.example")], length=len(CH) - 4 - 30) + DONE),
    ("M_4_then_hello", sl.handshake(1, b"", length=0) + SH),
    ("sni_L0", sl.client_hello([sl.extension(0)])),
    ("sni_L1", sl.client_hello([sl.extension(0, b"\x00"), ALPN])),
    ("sni_L4", sl.client_hello([sl.extension(0, b"\x00\x05\x00\x00")])),
    ("sni_L5", sl.client_hello([sl.extension(0, b"\x00\x02\x00\x00\x00")])),
    ("sni_L5_wants_more", sl.client_hello([sl.extension(0, b"\x00\x02\x00\x00\x07"), ALPN])),
    ("sni_cut_by_L", sl.client_hello([sl.sni(b"long.name.example", name_len=40), GROUPS])),
    ("sni_shorter_than_L", sl.client_hello([sl.sni(b"short.example.org", name_len=5)])),
    ("sni_first", sl.client_hello([sl.sni(b"first.example"), GROUPS, ALPN])),
    ("sni_middle", sl.client_hello([GROUPS, sl.sni(b"middle.example"), ALPN])),
    ("sni_last", sl.client_hello([GROUPS, ALPN, sl.sni(b"last.example")])),
    ("sni_twice", sl.client_hello([sl.sni(b"one.example"), GROUPS, sl.sni(b"two.example")])),
    ("sni_malformed_then_good", sl.client_hello([sl.extension(0, b"\x00\x00"), sl.sni(b"good.example")])),
    ("sni_non_ascii", sl.client_hello([sl.sni(b"n\xe4me\x00.example")])),
    ("no_extensions", sl.client_hello(None)),
    ("extensions_empty", sl.client_hello([])),
    ("extension_overruns", sl.client_hello([GROUPS, sl.extension(0, b"abc", length=900)])),
    ("ext_len_short", sl.client_hello([GROUPS, sl.sni(b"beyond.example")], ext_len=len(GROUPS) + 3)),
    ("session_id_32", sl.client_hello([sl.sni(b"sid.example")], sid=bytes(range(32)))),
    ("session_id_beyond_D", sl.client_hello(None)[:38] + b"\xf0\x01\x02\x03\x04"),
    ("many_ciphers", sl.client_hello([sl.sni(b"c.example")], ciphers=tuple(range(0x0A0A, 0x0A0A + 90)))),
    ("cipher_count_beyond_D", sl.client_hello(None)[:39] + b"\x7f\xfe\x00\x01"),
    ("v43_len0", sl.server_hello([sl.extension(43, b"")], version=0x0303)),
    ("v43_len2", sl.server_hello([sl.extension(43, b"\x03\x04")])),
    ("v43_len3", sl.server_hello([sl.extension(43, b"\x02\x03\x04")])),
    ("v43_len3_other", sl.server_hello([sl.extension(43, b"\x01\x03\x04")])),
    ("v43_len4", sl.server_hello([sl.extension(43, b"\x03\x04\x03\x03")])),
    ("v43_twice", sl.server_hello([sl.extension(43, b"\x7f\x1c"), sl.extension(43, b"\x03\x04")])),
    ("v43_behind_others", sl.server_hello([sl.extension(51, bytes(4)), sl.extension(43, b"\x03\x04")])),
    ("v43_in_client", sl.client_hello([sl.extension(43, b"\x02\x03\x04"), sl.sni(b"v.example")])),
    ("sni_in_server", sl.server_hello([sl.sni(b"ignored.example")])),
    ("server_no_extensions", sl.server_hello(None)),
    ("cipher_cut_D40", sl.server_hello(None)[:40]),
    ("cipher_cut_D41", sl.server_hello(None)[:41]),
    ("cipher_behind_sid", sl.server_hello(None, sid=bytes(8))),
    ("cipher_cut_behind_sid", sl.server_hello(None, sid=bytes(8))[:48]),
    ("server_D39", sl.server_hello(None)[:39]),
]


def record_types() -> list[bytes]:
    return [(srv if "server" in name else cli)(p, k) for k, (name, p) in enumerate(RECORD_TYPES)]


def hello_cases() -> list[bytes]:
    """Each HELLOS body as one handshake record whose length is the body's (a cut body: the record is cut too)."""
    return [cli(R(HS, body), k) for k, (_, body) in enumerate(HELLOS)]


def later_entries() -> list[bytes]:
    """Hellos in the 2nd and 3rd handshake entry, a hello in each of three, and handshake entries between others."""
    return [srv(R(HS, CERT) + R(HS, SH), 1), cli(R(HS, DONE) + R(CCS, b"\x01") + R(HS, CH), 2),
            srv(R(HS, CERT) + R(HS, DONE) + R(HS, SH13), 3), cli(R(HS, CH) + R(HS, SH) + R(HS, CH + SH), 4),
            cli(R(APP, bytes(20)) + R(HS, sl.handshake(8, b"") + CH) + R(HS, SH), 5)]


def many_records() -> list[bytes]:
    """1..13 records a packet: the first and the last a hello, app data between."""
    out = []
    for r in range(1, 14):
        recs = [R(HS, CH if r % 2 else SH)] + [R(APP, bytes(3 + j)) for j in range(r - 2)] + ([R(HS, SH)] if r > 1 else [])
        out.append(cli(b"".join(recs), r))
    return out


HOSTS = ("www.example.org", "cdn.example.net", "a.b.c.d.example.com", "x.io")
SUITES = (0xC02F, 0x1301, 0x0005, 0xC02B, 0x009C)


def ssl_k(k: int) -> bytes:
    """SSL packet k of the mixed batches: the packets of a handshake and its data in turn."""
    step = k % 6
    if step == 0:
        exts = [sl.sni(HOSTS[k % 4].encode() * (1 + k % 3)), GROUPS] + ([ALPN] if k % 5 else [])
        return cli(R(HS, sl.client_hello(exts, ciphers=tuple(range(2, 2 + k % 40)), sid=bytes(k % 33))), k)
    if step == 1:
        tls13 = [sl.extension(43, b"\x03\x04")] if k % 4 == 1 else []
        return srv(R(HS, sl.server_hello(tls13 + [sl.extension(0xFF01, b"\x00")], SUITES[k % 5])) + R(HS, CERT) +
                   R(HS, DONE), k)
    if step == 2:
        return cli(R(HS, sl.handshake(16, bytes(30 + k % 40))) + R(CCS, b"\x01") + R(HS, ENC), k)
    if step == 3:
        return srv(R(CCS, b"\x01") + R(HS, ENC), k)
    if step == 4:
        return cli(R(APP, bytes(j % 253 for j in range(20 + k % 200))), k)
    return srv(R(APP, bytes(10 + k % 90)) + (R(ALERT, b"\x01\x00") if k % 4 == 1 else b""), k)


def other_k(k: int) -> bytes:
    """A packet without an SSL layer: a TCP ACK on 443 or a payload on another port."""
    if k % 2:
        return sl.tcp_packet(b"", k, port=443)
    return sl.tcp_packet(bytes(1 + (k + j) % 250 for j in range(20 + k % 30)), k, port=4000 + k % 10)


HEAVY = cli(R(HS, CERT + sl.client_hello([GROUPS] * 40 + [sl.sni(b"heavy." * 20 + b"example")],
                                         ciphers=tuple(range(300)))) + R(HS, SH + CH), 7)


def heavy_slots(n: int) -> set:
    """Lane 0 and lane 63 of a tile, and the first and the last packet of every block."""
    at = {0} | ({(n // 64 - 1) * 64 + 63} if n >= 128 else set())
    for first in range(0, n, BLOCK):
        at |= {first, min(first + BLOCK, n) - 1}
    return at


def mixed(n: int, share: int) -> list[bytes]:
    """n packets with `share` per cent SSL; the heaviest packet of the cases (two hellos with names, in two entries)
    sits at the first and at the last lane of a tile and at both edges of every block."""
    step = {0: 0, 1: 97, 100: 1}[share]
    out = [ssl_k(k) if step and k % step == 0 else other_k(k) for k in range(n)]
    for k in heavy_slots(n) if n else ():
        out[k] = HEAVY
    return out


def heavy_count(n: int) -> int:
    return len(heavy_slots(n))


FLAG_BITS = (abi.F_NEEDS_HOST_L7, abi.F_NEEDS_HOST_PROTO, abi.F_DEPTH_OVERFLOW, abi.F_OVERSIZE, abi.F_BAD_DESC,
             abi.F_L7_KNOWN, abi.F_L7_SSL, abi.F_L7_HTTP)


def flag_combinations() -> list[int]:
    return [sum(b for j, b in enumerate(FLAG_BITS) if (m >> j) & 1) | (abi.F_IP_CSUM if m % 3 == 0 else 0)
            for m in range(256)]


def fuzz(count: int, seed: int) -> list[bytes]:
    """Seeded mutations of the crafted hello records: one to four changed bytes (random, a bit flip, a small length
    byte, a swap), a third of the records cut short with the record length left as it was."""
    rng = np.random.default_rng(seed)
    base = [body for _, body in HELLOS if len(body) >= 8]
    out = []
    for k in range(count):
        m = bytearray(base[int(rng.integers(len(base)))])
        for _ in range(int(rng.integers(1, 5))):
            at = int(rng.integers(len(m)))
            kind = int(rng.integers(4))
            if kind == 0:
                m[at] = int(rng.integers(256))
            elif kind == 1:
                m[at] ^= 1 << int(rng.integers(8))
            elif kind == 2:
                m[at] = int(rng.integers(6))
            else:
                to = int(rng.integers(len(m)))
                m[at], m[to] = m[to], m[at]
        cut = int(rng.integers(1, len(m) + 1)) if rng.integers(3) == 0 else len(m)
        out.append(cli(R(HS, bytes(m[:cut]), length=len(m)), k))
    return out


# ------------------------------------------------------------------ the families
OVERFLOWING = ("cap_sizing", "cap_sizing_names", "cap_msgs_short1", "cap_hellos_short1", "cap_names_short1",
               "cap_spec_short1")


def cases() -> list[Case]:
    out = [make("record_types", record_types()), make("hellos", hello_cases()), make("later_entries", later_entries()),
           make("many_records", many_records(), ml=16), make("fuzz", fuzz(400, 11)),
           make("fuzz_server", [srv(p[AT:], k) for k, p in enumerate(fuzz(150, 12))], kinds=2)]
    # rule 2 for every combination of the flags it reads, without and with recorded SSL entries: the flags win
    fl = flag_combinations()
    out.append(make("flags", [other_k(2 * k) for k in range(256)] + [ssl_k(k) for k in range(6)] * 2,
                    flags=fl + [0] * 6 + [0xFFFF, fl[1], fl[2], fl[4], fl[32], fl[37]]))
    # hand-made records: entries outside the packet, n_layers against max_layers, SSL as entry 0, no TCP in front, a
    # record type outside 20..23, a handshake entry whose hdr_len stops inside the hello
    p = cli(R(HS, CH) + R(APP, bytes(12)), 1)
    n_, at = len(p), AT
    r1 = 5 + len(CH)
    eth, ip4, tcp = (1, 2, 0, 14, n_), (2, 3, 14, 20, n_ - 14), (4, 4, 34, 20, n_ - 34)
    s = lambda o, hl, dl: (sl.P_SSL, 6, o, hl, dl)  # noqa: E731
    e1, e2 = s(at, r1, n_ - at), s(at + r1, 17, 17)
    odd = cli(b"\x18\x03\x03\x00\x02\x01\x02" + R(HS, SH), 2)  # a heartbeat record (type 24) in front
    lo = len(odd)
    chains = [
        [eth, ip4, tcp, e1, e2],                                # as the parse writes it
        [eth, ip4, tcp, s(at, r1, n_ - at + 1), e2],            # the first one byte past the packet: the second leads
        [eth, ip4, tcp, e1, s(at + r1, 17, 18)],
        [eth, ip4, tcp, s(at, r1, r1 - 1), e2],                 # hdr_len > data_len
        [eth, ip4, tcp, s(at, 4, n_ - at), s(at + r1, 4, 4)],   # hdr_len < 5, data_len < 5: none followed
        [eth, ip4, tcp, s(0xFFFF, 5, 5)],
        [eth, ip4, tcp, s(n_ - 5, 5, 5)],                       # the last five bytes
        [eth, ip4, tcp, s(at, 5, n_ - at)],                     # R = 0
        [eth, ip4, tcp, s(at, 5 + 43, n_ - at), e2],            # the record stops inside the hello: D = 43
        [e1, e2],                                               # SSL as entry 0: no TCP
        [eth, ip4, (5, 4, 34, 8, n_ - 34), e1, e2],             # UDP in front
        [eth, ip4, (4, 4, n_ - 3, 20, 3), e1],                  # the TCP entry's ports outside the packet
        [eth, ip4, (4, 4, n_ - 4, 20, 4), e1],                  # just inside
        [eth, ip4, tcp, (32, 7, at, 1, 1), e1],                 # something between TCP and SSL
        [eth, ip4, tcp, e1, (32, 7, at, 1, 1), e2],             # and between the SSL entries
        [eth, ip4, tcp, e1, e2],                                # n_layers 4: the second is not looked at
        [eth, ip4, tcp, e1, e2],                                # n_layers 3: NONE
        [eth, ip4, tcp, e1, e2],                                # n_layers 9 > max_layers: HOST
        [eth, ip4, tcp, e1, e2],                                # n_layers 0
    ]
    nl = [None] * 15 + [4, 3, 9, 0]
    odd_chain = [(1, 2, 0, 14, lo), (2, 3, 14, 20, lo - 14), (4, 4, 34, 20, lo - 34), s(at, 7, lo - at),
                 s(at + 7, lo - at - 7, lo - at - 7)]
    out.append(make("records", [p] * len(chains) + [odd], chains=chains + [odd_chain], n_layers=nl + [None]))
    for ml in (1, 3, 4, 5, 16):
        out.append(make(f"max_layers_{ml}", [ssl_k(k) for k in range(12)], ml=ml))
    # ports: the SSL port on either side, on both, and on neither
    ports = [cli(R(APP, bytes(8)), k, port) for k, port in enumerate((443, 993, 261, 995, 8443, 80))] + \
        [srv(R(APP, bytes(8)), k, port) for k, port in enumerate((443, 465, 8443))]
    both = bytearray(cli(R(APP, bytes(8)), 3, 443))
    both[34:36] = (993).to_bytes(2, "big")
    out.append(make("ports", ports + [bytes(both)],
                    chains=[None if int.from_bytes(q[34:36], "big") in sl.SSL_PORTS or
                            int.from_bytes(q[36:38], "big") in sl.SSL_PORTS else
                            [(1, 2, 0, 14, len(q)), (2, 3, 14, 20, len(q) - 14), (4, 4, 34, 20, len(q) - 34),
                             (sl.P_SSL, 6, AT, len(q) - AT, len(q) - AT)] for q in ports + [bytes(both)]]))
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
    out.append(parsed("parsed_mixed", mixed(200, 100) + record_types() + hello_cases() + later_entries()))
    out.append(parsed("parsed_ml3", mixed(64, 100), abi.make_opts(max_layers=3)))
    # batch shapes around the wave and block edges
    for n in SIZES:
        for share in SHARES:
            out.append(make(f"n{n}_s{share}", mixed(n, share)))
    out.append(make("n0", []))
    out.append(make("n65_brief", mixed(65, 100), use_brief=True))
    # every kinds value
    base = make("spec", mixed(70, 100) + hello_cases() + later_entries())
    for kinds in range(4):
        out.append(replace(base, name=f"kinds_{kinds}", kinds=kinds))
    # capacities
    cap = make("cap_exact", mixed(130, 100))
    m, k, nb = needs(cap)
    out += [cap,
            replace(cap, name="cap_sizing", out_msgs=0, out_hellos=0, names_cap=0, want_names=False, want_disp=False),
            replace(cap, name="cap_sizing_names", out_msgs=0, out_hellos=0, names_cap=0),
            replace(cap, name="cap_msgs_short1", out_msgs=m - 1),
            replace(cap, name="cap_hellos_short1", out_hellos=k - 1),
            replace(cap, name="cap_names_short1", names_cap=nb - 1),
            replace(cap, name="cap_spec_short1", max_msgs=m - 1),
            replace(cap, name="cap_spec_exact", max_msgs=m, out_msgs=m),
            replace(cap, name="cap_no_names", want_names=False, names_cap=0),
            replace(cap, name="cap_no_names_no_disp", want_names=False, want_disp=False, names_cap=0),
            replace(cap, name="cap_roomy", out_hellos=k + 7, names_cap=nb + 100)]
    return out
