"""Case generators and runners for pcppx_tlsfp_device / pcppx_tlsfp_reference (tests/test_tlsfp.py).

A Case is a source batch, its parse records (an input: written here the way the parse writes them -- one SSL layer per
TLS record behind Ethernet / IPv4 / TCP -- or crafted), the spec and the output's capacities. Three runners produce
the same Buffers from it -- model() (pcapplusplus_amd.tlsfp.model, the contract in plain Python with hashlib.md5),
run_reference() (pcppx_tlsfp_reference) and run_device() (pcppx_tlsfp_device) -- every buffer pre-filled with 0xA5 and
over-allocated, so equality of the whole buffers also shows that nothing beyond the output was touched, and nothing at
all but the totals on overflow.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

from pcapplusplus_amd import abi
from pcapplusplus_amd import tlsfp as tf

BLOCK = 1024  # source packets per block of the kernels (pcppx_internal.h kTlsfpBlockPk)
ML = 6        # max_layers of the cases' records, unless a case says otherwise
FILL, F64 = 0xA5, 0xA5A5A5A5A5A5A5A5
PAD_BYTES, PAD_ENTRIES = 64, 4
ETH = abi.LINKTYPE_ETHERNET
L7 = 54       # where the TCP payload of tf.tcp_packet() starts (IPv4)
NONE, CLIENT, SERVER, HOST, BAD = (abi.TLSFP_NONE, abi.TLSFP_CLIENT, abi.TLSFP_SERVER, abi.TLSFP_HOST,
                                   abi.TLSFP_BAD_DESC)


@dataclass
class Case:
    name: str
    data: np.ndarray      # u8
    offsets: np.ndarray   # u64
    caplens: np.ndarray   # u32
    summary: np.ndarray   # SUMMARY_DTYPE[n]: flags and n_layers are read
    layers: np.ndarray    # LAYER_DTYPE[n, ml]
    ml: int = ML
    client: bool = True
    server: bool = True
    max_hellos: int = 0
    max_recs: int | None = None   # None: n
    text_cap: int | None = None   # None: exactly what the texts need
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

    def maxr(self) -> int:
        return self.n if self.max_recs is None else self.max_recs

    def cap(self) -> int:
        if self.text_cap is not None:
            return self.text_cap
        return int(needs(self)[1])


@dataclass
class Buffers:
    recs: np.ndarray               # u8: (max_recs + PAD_ENTRIES) * 40 bytes
    text: np.ndarray | None        # u8
    disposition: np.ndarray | None
    totals: np.ndarray

    def records(self, k: int) -> np.ndarray:
        return self.recs[:k * 40].view(abi.TLSFP_REC_DTYPE)


FIELDS = ("recs", "text", "disposition")


def alloc(c: Case) -> Buffers:
    return Buffers(np.full((c.maxr() + PAD_ENTRIES) * 40, FILL, np.uint8),
                   np.full(c.cap() + PAD_BYTES, FILL, np.uint8) if c.want_text else None,
                   np.full(c.n + PAD_ENTRIES, FILL, np.uint8) if c.want_disp else None,
                   np.full(abi.TLSFP_TOTALS, F64, np.uint64))


# ------------------------------------------------------------------ runners
_MODEL: dict[tuple, tuple] = {}


def _result(c: Case, max_recs, text_cap) -> tf.Result:
    return tf.model(c.data, c.offsets, c.caplens, c.dlen(), c.summary["flags"], c.summary["n_layers"], c.layers, c.ml,
                    c.client, c.server, c.max_hellos, max_recs, text_cap, c.want_text)


def needs(c: Case) -> tuple[int, int]:
    """(records, text bytes) of the case's spec over its batch, whatever its capacities."""
    key = (id(c.data), id(c.offsets), id(c.caplens), id(c.layers), id(c.summary), c.ml, c.client, c.server, c.data_len)
    if key not in _MODEL:
        r = tf.model(c.data, c.offsets, c.caplens, c.dlen(), c.summary["flags"], c.summary["n_layers"], c.layers, c.ml,
                     c.client, c.server)
        _MODEL[key] = (len(r.recs), len(r.text), c)  # c kept alive: the ids stay its own
    return _MODEL[key][:2]


def model(c: Case) -> Buffers:
    """include/pcppx.h's tlsfp contract, restated in pcapplusplus_amd/tlsfp.py, as the buffers a call leaves."""
    out = alloc(c)
    r = _result(c, c.maxr(), c.cap())
    out.totals[:] = r.totals
    if r.disposition is None:
        return out
    if out.disposition is not None:
        out.disposition[:c.n] = r.disposition
    out.recs[:len(r.recs) * 40] = tf.records_array(r.recs).view(np.uint8)
    if out.text is not None:
        out.text[:len(r.text)] = np.frombuffer(r.text, np.uint8)
    return out


def spec_of(c: Case) -> abi.TlsfpSpec:
    return abi.make_tlsfp_spec(c.client, c.server, c.max_hellos)


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
    o = abi.Tlsfps(out.recs.ctypes.data, opt(out.text), c.cap(), opt(out.disposition), c.maxr(), 0,
                   out.totals.ctypes.data)
    abi.tlsfp_reference(b, r, c.ml, spec_of(c), o)
    del rec, lay
    return out


class DeviceRun:
    """A case's tensors on the device; launch() queues pcppx_tlsfp_device on a stream, result() reads the buffers."""

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
        self.d_recs = self.up(host.recs)
        self.d_text = None if host.text is None else self.up(host.text)
        self.d_disp = None if host.disposition is None else self.up(host.disposition)
        self.d_tot = self.up(host.totals.view(np.int64))

    def up(self, a: np.ndarray):
        import torch

        return torch.from_numpy(a).to(self.device)

    def launch(self, engine, stream: int) -> None:
        c = self.c
        engine.tlsfp_device(self.data, self.offsets, self.caplens, c.n, ETH, self.layers, c.ml, spec_of(c), self.d_recs,
                            self.d_tot, c.maxr(), self.d_text, c.cap(), self.d_disp, stream, data_len=self.data_len,
                            summary=self.summary, brief=self.brief)

    def result(self) -> Buffers:
        import torch

        torch.cuda.synchronize(self.device)
        down = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
        return Buffers(down(self.d_recs), down(self.d_text), down(self.d_disp), down(self.d_tot).view(np.uint64))


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
    """The all-or-nothing rule: the records, the text and the dispositions still hold the fill, every byte of them."""
    for f in FIELDS:
        g = getattr(got, f)
        assert g is None or bool((g == FILL).all()), (what, f)


# ------------------------------------------------------------------ records
def ssl_layers(pkt: bytes, start: int = L7) -> list[tuple]:
    """The chain the parse records for an Ethernet / IPv4 / TCP packet with TLS records from `start`: one SSL layer per
    record, its header length the record's length as the capture clamps it (SSLLayer.cpp:126-149)."""
    chain = [(1, 2, 0, 14, len(pkt)), (2, 3, 14, 20, len(pkt) - 14), (4, 4, 34, 20, len(pkt) - 34)]
    at = start
    while len(pkt) - at >= 5:
        left = len(pkt) - at
        hdr = min(5 + ((pkt[at + 3] << 8) | pkt[at + 4]), left)
        chain.append((tf.P_SSL, 7, at, hdr, left))
        at += hdr
    return chain


def make(name: str, packets: list[bytes], chains: list | None = None, flags: list | None = None, ml: int = ML,
         n_layers: list | None = None, **kw) -> Case:
    """A case over the packets back to back. chains[i]: packet i's layer entries (None: ssl_layers of it), of which the
    first ml are recorded; n_layers[i] (None: the chain's length capped at ml, as the parse caps it)."""
    n = len(packets)
    caps = np.array([len(p) for p in packets], np.uint32)
    offs = (np.cumsum(caps, dtype=np.uint64) - caps).astype(np.uint64)
    data = np.frombuffer(b"".join(packets) + b"\0", np.uint8).copy()
    summary = np.zeros(n, abi.SUMMARY_DTYPE)
    layers = np.zeros((n, ml), abi.LAYER_DTYPE)
    for i, p in enumerate(packets):
        chain = ssl_layers(p) if chains is None or chains[i] is None else chains[i]
        for k, e in enumerate(chain[:ml]):
            layers[i, k] = e
        summary["n_layers"][i] = min(len(chain), ml) if n_layers is None or n_layers[i] is None else n_layers[i]
        over = abi.F_DEPTH_OVERFLOW if len(chain) > ml else 0
        summary["flags"][i] = over if flags is None or flags[i] is None else flags[i]
    return Case(name, data, offs, caps, summary, layers, ml=ml, **kw)


# ------------------------------------------------------------------ packets
GROUPS = tf.groups_ext([29, 23, 24])
FORMATS = tf.formats_ext([0, 1, 2])
EXTS = tf.ext(0, b"\0\x05\0\0\x02ab") + tf.ext(23) + GROUPS + FORMATS + tf.ext(65281, b"\0") + tf.ext(43, b"\x02\x03\x04")
CH = tf.client_hello(ciphers=(0x1301, 0x1302, 0xC02F, 0x009C, 0x000A), extensions=EXTS, sid=bytes(range(32)))
SH = tf.server_hello(cipher=0xC02F, extensions=tf.ext(65281, b"\0") + tf.ext(11, b"\x01\0") + tf.ext(23), sid=b"\x07" * 32)
SH13 = tf.server_hello(extensions=tf.ext(51, b"\0\x1d\0\x02ab") + tf.ext(43, b"\x03\x04"))


def pk(payload: bytes, k: int = 0, from_server: bool = False) -> bytes:
    return tf.tcp_packet(payload, k, from_server)


def hs(*msgs: bytes, **kw) -> bytes:
    return tf.record(b"".join(msgs), **kw)


def ch_k(k: int) -> bytes:
    """A ClientHello whose fingerprint depends on k % 40."""
    return tf.client_hello(ciphers=(0x1301, 0xC000 + k % 40, 0x0A0A), extensions=EXTS)


def sh_k(k: int) -> bytes:
    return tf.server_hello(cipher=0xC000 + k % 7, extensions=tf.ext(43, b"\x03\x04") + tf.ext(51, b"\0\x1d\0\x01a"))


def ack(k: int) -> bytes:
    return pk(b"", k)


def app(k: int, size: int = 40) -> bytes:
    return pk(tf.record(bytes(1 + (k + j) % 250 for j in range(size)), tf.APPLICATION_DATA), k)


def bounds() -> list[bytes]:
    """R and D at 3 .. 41 for both hellos: the record cut short, the message longer than what is left of it."""
    out = []
    for at in (3, 4, 5, 6, 15, 16, 38, 39, 40, 41):
        for msg in (CH, SH):
            out.append(pk(tf.record(msg[:at])))                           # R = at
            out.append(pk(tf.record(tf.other_message(11, 4) + msg[:at])))  # D = at behind an 8-byte message
    out.append(pk(tf.record(CH, length=len(CH) + 100)))   # a record longer than the capture
    out.append(pk(tf.record(CH))[:-10])                   # ... and a capture that cuts the record
    out.append(pk(tf.record(SH, length=len(SH) + 3000)))
    for D in (15, 16, 17):  # the unknown rule, on both sides of D = 16
        out.append(pk(tf.record(tf.client_hello(length=0x10000 + 60)[:D])))      # length1 >= 1
        out.append(pk(tf.record(bytes(5) + CH[:D - 5])))                         # five zero bytes
        out.append(pk(tf.record(tf.other_message(11, 4) + tf.server_hello(length=0x20000)[:D])))
    return out


def order() -> list[bytes]:
    return [
        pk(hs(tf.other_message(11, 20), CH)),                   # a hello behind another message
        pk(hs(tf.other_message(12, 9), tf.other_message(14, 0), SH), 1, True),
        pk(hs(SH, CH), 2),                                      # both in one record: ClientHello wins when asked for
        pk(hs(CH, SH), 3),
        pk(hs(SH, SH13, CH, CH), 4),                            # the first of each type
        pk(hs(tf.other_message(11, 20)) + hs(CH), 5),           # a hello in a second handshake record: not found
        pk(tf.record(b"\x01", tf.CHANGE_CIPHER_SPEC) + hs(CH), 6),  # a handshake record behind another record: found
        pk(tf.record(b"\x01", tf.CHANGE_CIPHER_SPEC) + app(0)[L7:] + hs(SH), 7, True),
        pk(hs(tf.other_message(11, 20)), 8),                    # no hello at all
        app(9),
        ack(10),
    ]


def client_fields() -> list[bytes]:
    g = 0x0A0A
    cut_m = tf.client_hello(extensions=EXTS, length=len(tf.client_hello(extensions=EXTS)) - 4 - 9)
    full = tf.client_hello(extensions=EXTS)
    msgs = [
        tf.client_hello(sid=b"s" * 10, sid_len=200)[:52],               # a session id clamped by D
        tf.client_hello(sid=b"s" * 10, sid_len=200),
        tf.client_hello(ciphers=(1, 2, 3, 4), cipher_bytes=400, with_extensions=False),  # a cipher count past D
        tf.client_hello(ciphers=(1, 2, 3, 4), cipher_bytes=400, extensions=EXTS),
        tf.client_hello(ciphers=(1, 2, 3), cipher_bytes=5, extensions=EXTS),             # an odd cipher-list length
        tf.client_hello(ciphers=(1, 2, 3), cipher_bytes=7, extensions=EXTS),
        cut_m + b"\x01" * 9,                                              # an extension list cut by M (D is larger)
        cut_m,
        full[:-3],                                                        # ... and by D
        full[:-1],
        tf.client_hello(extensions=EXTS, ext_len=len(EXTS) - 2),          # ... and by its own length
        tf.client_hello(extensions=EXTS, ext_len=len(EXTS) + 50),
        tf.client_hello(extensions=tf.ext(23) + tf.ext(5, b"abc", length=50)),  # an extension longer than what is left
        tf.client_hello(extensions=tf.ext(23) + tf.ext(5, b"", length=0xFFFC)),
        tf.client_hello(extensions=tf.ext(23) + tf.ext(65281) + tf.ext(35)),    # zero-length extensions
        tf.client_hello(extensions=tf.ext(23) + b"\0\x0a\0"),                   # three bytes left
        tf.client_hello(ciphers=(g, 0x1301, 0x1A1A, 0xFAFA, 0x0A1A, 0x1A0A, 0x0B0B, 0xAAAA),  # GREASE in every list
                        extensions=tf.ext(0x2A2A) + tf.groups_ext([0x3A3A, 29, 0x4A4A, 23, 0xBABA]) + FORMATS +
                        tf.ext(0xCACA, b"\0")),
        tf.client_hello(ciphers=(g, 0xEAEA), extensions=tf.ext(0x5A5A) + tf.groups_ext([0x6A6A])),  # nothing is left
        tf.client_hello(extensions=tf.groups_ext([29, 23]) + tf.groups_ext([24]) + tf.formats_ext([2]) +
                        tf.formats_ext([0])),                                    # two of each: the first wins
        tf.client_hello(extensions=tf.groups_ext([29, 23], list_len=6) + tf.groups_ext([24])),  # malformed groups
        tf.client_hello(extensions=tf.ext(10, b"\0\x03abc") + FORMATS),
        tf.client_hello(extensions=tf.ext(10, b"\0") + tf.ext(10, b"") + FORMATS),
        tf.client_hello(extensions=tf.ext(10, b"\0\0") + FORMATS),
        tf.client_hello(extensions=GROUPS + tf.formats_ext([0, 1], list_len=5)),  # malformed formats
        tf.client_hello(extensions=GROUPS + tf.ext(11, b"") + FORMATS),
        tf.client_hello(extensions=GROUPS + tf.formats_ext([], list_len=0)),
        tf.client_hello(extensions=GROUPS + tf.formats_ext([255, 100, 9])),
        tf.client_hello(extensions=EXTS, compression=b""),                # zero and two compression methods: the quirk
        tf.client_hello(extensions=EXTS, compression=b"\0\x01"),
        tf.client_hello(ciphers=(), extensions=EXTS),
        tf.client_hello(with_extensions=False),
        tf.client_hello(version=0x0301, ciphers=(65535, 0, 9, 10, 99, 100, 999, 1000, 9999, 10000), extensions=b""),
    ]
    return [pk(hs(m), k) for k, m in enumerate(msgs)]


def server_fields() -> list[bytes]:
    v = lambda d: tf.ext(EXT_V, d)  # noqa: E731
    msgs = [
        tf.server_hello(extensions=v(b"") + tf.ext(51)),                     # supported_versions of 0, 2, 3, 3, 4 bytes
        tf.server_hello(extensions=tf.ext(51) + v(b"\x03\x04")),
        tf.server_hello(extensions=v(b"\x02\x03\x04")),
        tf.server_hello(extensions=v(b"\x04\x03\x04")),
        tf.server_hello(extensions=v(b"\x03\x04\x03\x03")),
        tf.server_hello(extensions=v(b"\x7f\x1c") + v(b"\x03\x04")),         # the first one decides
        tf.server_hello(extensions=v(b"\x03") + v(b"\x03\x04")),
        tf.server_hello(cipher=0x0A0A, extensions=tf.ext(0x3A3A) + v(b"\x03\x04") + tf.ext(0xFAFA, b"x")),  # GREASE kept
        tf.server_hello(version=0x0302, with_extensions=False),
        tf.server_hello(sid=b"i" * 32, extensions=tf.ext(65281, b"\0"))[:-2],
        tf.server_hello(sid=b"i" * 32)[:75],
        tf.server_hello(extensions=tf.ext(23) + tf.ext(35), length=44),      # the list cut by M
        SH, SH13,
    ]
    return [pk(hs(m), k, True) for k, m in enumerate(msgs)]


EXT_V = tf.EXT_VERSIONS
TEXT_LENGTHS = (55, 56, 63, 64, 65, 119, 120, 128)


def ch_with_text_len(want: int) -> bytes:
    """A ClientHello without extensions whose text "771,<ciphers>,,," has exactly `want` bytes."""
    by_width = {1: 5, 2: 47, 3: 156, 4: 4865, 5: 49195}
    ciphers, left = [], want - len("771,,,,")
    while left > 0:
        room = left - (1 if ciphers else 0)  # the '-' in front
        w = min(5, room)
        if room - w == 1:  # a lone '-' cannot follow
            w -= 1
        ciphers.append(by_width[w])
        left = room - w
    return tf.client_hello(ciphers=ciphers, with_extensions=False)


def text_lengths() -> list[bytes]:
    return [pk(hs(ch_with_text_len(n)), n) for n in TEXT_LENGTHS]


def longest() -> list[bytes]:
    """One ClientHello of caplen 65,535 filled with cipher entries."""
    count = (65535 - L7 - 5 - len(tf.client_hello(ciphers=(), with_extensions=False))) // 2
    p = pk(hs(tf.client_hello(ciphers=[49195 + k % 7 for k in range(count)], with_extensions=False), b"\x01"))
    assert len(p) == 65535, len(p)
    return [p]


def mixed(n: int, first: int = 0) -> list[bytes]:
    """ClientHello, ServerHello and application data in turn."""
    out = []
    for i in range(first, first + n):
        out.append(pk(hs(ch_k(i)), i) if i % 3 == 0 else pk(hs(sh_k(i)), i, True) if i % 3 == 1 else app(i))
    return out


EDGES = (0, 1, 62, 63, 64, 65, 127, 128, 255, 256, 511, 512, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 2099)


def edges() -> list[bytes]:
    """Hellos only on both sides of every wave and block edge, bare ACKs between them."""
    return [pk(hs(ch_k(i) if i % 2 else sh_k(i)), i, i % 2 == 0) if i in EDGES else ack(i) for i in range(2100)]


def flag_cases() -> Case:
    """Records and flags over one ClientHello packet: what decides between HOST and NONE, and records that point
    outside the packet."""
    p = pk(hs(CH))
    good = ssl_layers(p)
    ssl = good[3]
    no_ssl = good[:3]
    F = abi
    rows = [  # (chain, flags, n_layers)
        (good, 0, None), (good, F.F_DEPTH_OVERFLOW, None), (no_ssl, F.F_DEPTH_OVERFLOW, None),
        (no_ssl, 0, None), (no_ssl, F.F_TRAILER | F.F_IP_CSUM | F.F_L4_CSUM_OK, None),
        (no_ssl, F.F_NEEDS_HOST_L7, None), (no_ssl, F.F_NEEDS_HOST_L7 | F.F_L7_KNOWN, None),
        (no_ssl, F.F_NEEDS_HOST_L7 | F.F_L7_KNOWN | F.F_L7_SSL, None),
        (no_ssl, F.F_NEEDS_HOST_L7 | F.F_L7_KNOWN | F.F_L7_HTTP, None),
        (no_ssl, F.F_NEEDS_HOST_L7 | F.F_L7_KNOWN | F.F_L7_DNS, None), (no_ssl, F.F_NEEDS_HOST_L7 | F.F_L7_SSL, None),
        (no_ssl, F.F_L7_KNOWN | F.F_L7_SSL, None), (no_ssl, F.F_NEEDS_HOST_PROTO, None), (no_ssl, F.F_OVERSIZE, None),
        (no_ssl, F.F_BAD_DESC, None), (good, F.F_NEEDS_HOST_PROTO | F.F_NEEDS_HOST_L7, None),
        (no_ssl, 0, ML + 1), (good, 0, 3), (good, 0, 0), (good, 0, 255),
    ]
    off, hdr, dlen = ssl[2], ssl[3], ssl[4]
    for o, h, d in ((off, hdr, dlen + 1), (off + 1, hdr, dlen), (off, dlen + 1, dlen), (off, 4, dlen), (off, 5, dlen),
                    (off, 8, dlen), (off, hdr, 4), (off, 3, 3), (65535, hdr, dlen), (off, 65535, 65535),
                    (len(p) - 5, 5, 5), (len(p) - 4, 5, 5), (off - 1, hdr, dlen), (0, 14, len(p))):
        bad = (tf.P_SSL, 7, o, h, d)
        rows.append((no_ssl + [bad], 0, None))        # an entry that is not followed ...
        rows.append((no_ssl + [bad, ssl], 0, None))   # ... and the next one is looked at
    rows.append((no_ssl + [(17, 7, off, hdr, dlen)], 0, None))  # another protocol at the same place
    rows.append(([ssl], 0, None))
    c = make("flags", [p] * len(rows), [r[0] for r in rows], [r[1] for r in rows], n_layers=[r[2] for r in rows])
    return c


def descriptors() -> Case:
    """Bad descriptors, caplen 0 and gaps between hellos."""
    c = make("descriptors", mixed(80))
    offs, caps = c.offsets.copy(), c.caplens.copy()
    offs[5] = len(c.data) - 1                    # past the end
    caps[11] = 0xFFFFFFF0                        # a huge caplen
    offs[17] = np.uint64(0xFFFFFFFFFFFFFFF0)     # the end wraps 64 bits
    offs[21], caps[21] = len(c.data), 0          # an empty packet at the very end is in bounds ...
    offs[22], caps[22] = len(c.data), 1          # ... one byte there is not
    caps[30] = 0                                 # caplen 0 with its records left as they were
    caps[33] -= 1                                # a hello cut by one byte: its layers now end outside it
    caps[36] = L7 + 4                            # cut inside the record header
    return replace(c, offsets=offs, caplens=caps)


def cases() -> list[Case]:
    out = [
        make("bounds", bounds()), make("order", order()), make("client_fields", client_fields()),
        make("server_fields", server_fields()), make("text_lengths", text_lengths()), make("longest", longest()),
        flag_cases(), descriptors(),
        make("max_layers_1", order(), ml=1),             # the SSL layer is cut off: HOST
        make("max_layers_4", order(), ml=4),             # only the first record's layer is there
        make("max_layers_16", order(), ml=16),
        make("edges", edges()), make("all_hellos", [pk(hs(ch_k(i)), i) if i % 2 else pk(hs(sh_k(i)), i, True) for i in range(1300)]),
        make("no_hellos", [app(i) if i % 2 else ack(i) for i in range(1100)]),
    ]
    out += [make(f"n{n}", mixed(n)) for n in (0, 1, 63, 64, 65, 1024, 1025)]
    both = make("kinds", order() + bounds() + mixed(70))
    out += [replace(both, name="kinds_ch", server=False), replace(both, name="kinds_sh", client=False), both]
    base = make("cap", mixed(200))
    k, nb = needs(base)
    out += [
        replace(base, name="cap_exact", max_recs=k, text_cap=nb, max_hellos=k),
        replace(base, name="cap_recs_short1", max_recs=k - 1),
        replace(base, name="cap_text_short1", text_cap=nb - 1),
        replace(base, name="cap_hellos_short1", max_hellos=k - 1),
        replace(base, name="cap_no_text", want_text=False, text_cap=0),
        replace(base, name="cap_no_text_no_disp", want_text=False, want_disp=False, max_recs=k),
        replace(base, name="cap_sizing", max_recs=0, want_text=False, want_disp=False),
        replace(base, name="cap_sizing_text", max_recs=0, text_cap=0),
    ]
    out += [replace(c, name=c.name + "_brief", use_brief=True) for c in list(out)]
    return out


OVERFLOWING = {n + s for n in ("cap_recs_short1", "cap_text_short1", "cap_hellos_short1", "cap_sizing", "cap_sizing_text")
               for s in ("", "_brief")}
