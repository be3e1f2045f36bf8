"""HTTP messages in plain Python: builders, the independent model of the http contract, the per-field rows and
HttpAnalyzer's tables.

HttpRequestFirstLine / HttpResponseFirstLine parse a message's first line and TextBasedProtocolMessage::parseFields
links one HeaderField per header line (Packet++/src/HttpLayer.cpp:166-320, :850-985, TextBasedProtocol.cpp:87-139,
:448-541); Examples/HttpAnalyzer reads the method, the Host value, the status, Content-Type, Content-Length and the
header size of every packet. pcppx_http_device / pcppx_http_reference produce one record per message and per field the
caller asks for (include/pcppx.h, http). This module holds

  request() / response() / tcp_packet()
             crafted messages and packets for the tests and the benchmark,
  model()    the http contract restated packet by packet over Python byte strings with bytes.find: it shares no code
             with the C++ / HIP implementation and is what the tests compare pcppx_http_reference with,
  rows()     messages, field records and text turned into one row per field record,
  analyze()  HttpAnalyzer's tables from the records of a call with ANALYZE_NAMES and text 3.
"""
from __future__ import annotations

import re
import struct
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from . import abi

P_REQUEST, P_RESPONSE = 6, 7  # pcpp::HTTPRequest, pcpp::HTTPResponse
ANALYZE_NAMES = ("host", "user-agent", "content-type", "content-length")  # what analyze() reads


# ------------------------------------------------------------------ builders
def _headers(headers, eol: bytes) -> bytes:
    out = b""
    for h in headers:
        if isinstance(h, (bytes, bytearray)):
            out += bytes(h)  # a raw line, line end included
        else:
            out += h[0].encode("latin-1") + b": " + h[1].encode("latin-1") + eol
    return out


def request(method: str = "GET", uri: str = "/", headers=(), version: str = "1.1", body: bytes = b"",
            eol: bytes = b"\r\n", end: bool = True) -> bytes:
    """A request: the first line, the headers ((name, value) pairs or raw lines), the empty line (end) and a body."""
    return f"{method} {uri} HTTP/{version}".encode("latin-1") + eol + _headers(headers, eol) + (eol if end else b"") + body


def response(code: int = 200, message: str = "OK", headers=(), version: str = "1.1", body: bytes = b"",
             eol: bytes = b"\r\n", end: bool = True) -> bytes:
    return f"HTTP/{version} {code:03d} {message}".encode("latin-1") + eol + _headers(headers, eol) + \
        (eol if end else b"") + body


_MAC = bytes.fromhex("020000000001020000000002")


def tcp_packet(payload: bytes, k: int = 0, from_server: bool = False, port: int = 80) -> bytes:
    """Ethernet / IPv4 / TCP around a payload, client port 40000 + k % 1000; the payload starts at byte 54."""
    ca, sa = 0x0A000000 + 1 + k % 250, 0xC0A80001 + (k // 250) % 250
    src, dst = (sa, ca) if from_server else (ca, sa)
    cp = 40000 + k % 1000
    sport, dport = (port, cp) if from_server else (cp, port)
    tcp = struct.pack(">HHIIBBHHH", sport, dport, 1000 + k, 2000 + k, 0x50, 0x18, 512, 0, 0) + payload
    return _MAC + b"\x08\x00" + struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(tcp), k & 0xFFFF, 0x4000, 64, 6, 0, src,
                                            dst) + tcp


# ------------------------------------------------------------------ the contract (include/pcppx.h, http), restated
@dataclass
class FirstLine:
    length: int
    complete: bool = False
    method: int = abi.HTTP_METHOD_UNKNOWN
    version: int = abi.HTTP_VERSION_UNKNOWN
    a: tuple | None = None  # (offset, length) of the URI / the status message
    status: int = 0


def _version(text: bytes) -> int:
    t = text.decode("latin-1")
    return abi.HTTP_VERSIONS.index(t) if t in abi.HTTP_VERSIONS else abi.HTTP_VERSION_UNKNOWN


def request_line(d: bytes) -> FirstLine:
    """Rule 4."""
    L = len(d)
    sp = d.find(b" ")
    name = d[:sp].decode("latin-1") if sp > 0 else ""
    if L < 4 or name not in abi.HTTP_METHODS:
        return FirstLine(L)
    method, u = abi.HTTP_METHODS.index(name), sp + 1
    v = d.find(b" HTTP/", u)
    if v < 0 or v + 9 > L:
        return FirstLine(L, method=method)
    e = d.find(b"\n", v + 6)
    return FirstLine(L if e < 0 else e + 1, e >= 0, method, _version(d[v + 6:v + 9]), (u, v - u))


def response_line(d: bytes) -> FirstLine:
    """Rule 5."""
    L = len(d)
    version = _version(d[5:8]) if L >= 8 and d.startswith(b"HTTP/") else abi.HTTP_VERSION_UNKNOWN
    e0 = d.find(b"\n")
    r = FirstLine(L if e0 < 0 else e0 + 1, e0 >= 0, version=version)
    if version == abi.HTTP_VERSION_UNKNOWN or L < 12 or not re.fullmatch(rb"[0-9]{3}", d[9:12]):
        return r
    e = d.find(b"\n", 13)
    if e < 0:
        return r
    msg = d[13:e]
    if msg.endswith(b"\r"):
        msg = msg[:-1]
    if msg:
        r.status, r.a = int(d[9:12]), (13, len(msg))
    return r


@dataclass
class Field:
    off: int
    size: int
    end: bool
    name_len: int = 0
    value: tuple | None = None  # (offset, length)


def field_at(d: bytes, off: int) -> Field:
    """Rule 6."""
    L = len(d)
    e = d.find(b"\n", off)
    if e < 0:
        z = d.find(b"\0", off)
        size = (L if z < 0 else z) - off
    else:
        size = e - off + 1
    if size == 0 or d[off:off + 1] in (b"\r", b"\n"):
        return Field(off, size, True)
    c = d.find(b":", off)
    if c < 0 or (e >= 0 and c >= e):
        return Field(off, size, False, size)
    f = Field(off, size, False, c - off)
    vp = c + 1
    while vp < L and d[vp] == 0x20:
        vp += 1
    if vp < L:
        f.value = (vp, L - vp if e < 0 else e - vp - (1 if d[e - 1] == 0x0D else 0))
    return f


def linked_fields(d: bytes, first_line_len: int) -> list:
    """Rule 7: every linked field, the end-of-header one included."""
    L = len(d)
    out = [field_at(d, first_line_len)]
    while not out[-1].end and out[-1].off + out[-1].size < L:
        nxt = field_at(d, out[-1].off + out[-1].size)
        if nxt.size == 0:
            break
        out.append(nxt)
    return out


def atoi(value: bytes):
    """Rule 9: (the number, out of an int's range)."""
    m = re.match(rb"[ \t\n\v\f\r]*([+-]?)([0-9]*)", value.split(b"\0")[0])
    mag = int(m.group(2) or b"0")
    if mag > 0x7FFFFFFF:
        return 0, True
    return (-mag if m.group(1) == b"-" else mag), False


def http_layer(cap: int, layers, n_layers: int, max_layers: int):
    """Rule 2 without the kinds: None without an entry of proto 6 / 7; else (offset, L, kind), or False for an entry
    that is not followed."""
    for k in range(min(n_layers, max_layers)):
        e = layers[k]
        if int(e["proto"]) not in (P_REQUEST, P_RESPONSE):
            continue
        o, h, L = int(e["offset"]), int(e["hdr_len"]), int(e["data_len"])
        return (o, L, int(e["proto"]) - P_REQUEST) if h <= L and o + L <= cap else False
    return None


def needs_host(flags: int, n_layers: int, max_layers: int) -> bool:
    """Rule 3."""
    if flags & (abi.F_NEEDS_HOST_PROTO | abi.F_OVERSIZE | abi.F_BAD_DESC | abi.F_DEPTH_OVERFLOW):
        return True
    if n_layers > max_layers:
        return True
    return bool(flags & abi.F_NEEDS_HOST_L7) and (bool(flags & abi.F_L7_HTTP) or not flags & abi.F_L7_KNOWN)


@dataclass
class Message:
    index: int
    layer_offset: int
    kind: int
    d: bytes
    line: FirstLine
    fields: list  # the linked fields that are not end-of-header
    header_len: int
    flags: int
    content_length: int


def message(index: int, layer_offset: int, kind: int, d: bytes) -> Message:
    """Rules 4-9 over the layer's bytes."""
    line = request_line(d) if kind == abi.HTTP_REQUEST else response_line(d)
    linked = linked_fields(d, line.length)
    last = linked[-1]
    flags = (abi.HTTP_FIRST_LINE_COMPLETE if line.complete else 0) | \
        (abi.HTTP_HEADER_COMPLETE if last.end or last.name_len == 0 else 0)
    fields = [f for f in linked if not f.end]
    cl = 0
    for f in fields:
        if d[f.off:f.off + f.name_len].lower() == b"content-length":
            cl, rng = atoi(d[f.value[0]:f.value[0] + f.value[1]] if f.value else b"")
            flags |= abi.HTTP_HAS_CONTENT_LENGTH | (abi.HTTP_CONTENT_LENGTH_RANGE if rng else 0)
            break
    return Message(index, layer_offset, kind, d, line, fields, last.off + last.size, flags, cl)


def _lower(b: bytes) -> bytes:
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in b)


@dataclass
class Result:
    """What a call writes: totals always; the rest None / empty on overflow."""
    totals: list
    disposition: list | None = None
    msgs: list = field(default_factory=list)    # rows of abi.HTTP_MSG_DTYPE
    fields: list = field(default_factory=list)  # rows of abi.HTTP_FIELD_DTYPE
    text: bytes = b""
    messages: list = field(default_factory=list)  # the Message objects, whatever the capacities


def model(data, offsets, caplens, data_len: int, flags, n_layers, layers, max_layers: int, names=(),
          fields: int = abi.HTTP_FIELDS_WANTED, text: int = 3, kinds: int = 3, max_msgs: int = 0,
          out_msgs: int | None = None, out_fields: int | None = None, text_cap: int | None = None,
          want_text: bool = True) -> Result:
    """The http contract over a batch: data (u8 array), the descriptors, the records' flags / n_layers columns and the
    FIXED layer array [n, max_layers]; names: the spec's, as bytes. out_msgs / out_fields / text_cap None: always
    enough."""
    n = len(caplens)
    names = [nm.encode("latin-1") if isinstance(nm, str) else bytes(nm) for nm in names]
    disp, found = [], []
    for i in range(n):
        off, cap = int(offsets[i]), int(caplens[i])
        if off + cap > data_len:
            disp.append(abi.HTTP_BAD_DESC)
            continue
        lay = http_layer(cap, layers[i], int(n_layers[i]), max_layers)
        if lay is None:
            disp.append(abi.HTTP_HOST if needs_host(int(flags[i]), int(n_layers[i]), max_layers) else abi.HTTP_NONE)
            continue
        if lay is False or not (kinds >> lay[2]) & 1:
            disp.append(abi.HTTP_NONE)
            continue
        o, L, kind = lay
        found.append(message(i, o, kind, bytes(data[off + o:off + o + L])))
        disp.append(abi.HTTP_MSG)
    msgs, recs, out = [], [], bytearray()
    for j, m in enumerate(found):
        d, first, pos0, seen = m.d, len(recs), len(out), set()
        if text & abi.HTTP_TEXT_FIRST_LINE and m.line.a:
            out += d[m.line.a[0]:m.line.a[0] + m.line.a[1]]
        for f in m.fields:
            low = _lower(d[f.off:f.off + f.name_len])
            nid = names.index(low) if low in names else abi.HTTP_NO_NAME
            if fields == abi.HTTP_FIELDS_NONE or (fields == abi.HTTP_FIELDS_WANTED and nid == abi.HTTP_NO_NAME):
                continue
            fl = abi.HTTP_HAS_VALUE if f.value else 0
            tl = 0
            at = len(out)
            if nid != abi.HTTP_NO_NAME:
                if nid not in seen:
                    fl |= abi.HTTP_FIRST
                seen.add(nid)
                if text & abi.HTTP_TEXT_VALUES and f.value:
                    out += d[f.value[0]:f.value[0] + f.value[1]]
                    tl = f.value[1]
            vo, vl = f.value or (0, 0)
            recs.append((at, j, f.off, f.name_len, vo, vl, tl, nid, fl))
        a = m.line.a or (0, 0)
        msgs.append((first, pos0, m.index, m.content_length, m.layer_offset, len(d), m.header_len, m.line.length,
                     len(m.fields), len(recs) - first, a[0], a[1], m.line.status, len(out) - pos0, m.kind,
                     m.line.method, m.line.version, m.flags))
    totals = [0] * abi.HTTP_TOTALS
    totals[abi.HTTP_MSGS] = len(found)
    totals[abi.HTTP_REQUESTS] = sum(1 for m in found if m.kind == abi.HTTP_REQUEST)
    totals[abi.HTTP_RESPONSES] = sum(1 for m in found if m.kind == abi.HTTP_RESPONSE)
    totals[abi.HTTP_FIELDS] = len(recs)
    totals[abi.HTTP_TEXT_BYTES] = len(out)
    totals[abi.HTTP_HOST_N] = disp.count(abi.HTTP_HOST)
    totals[abi.HTTP_BAD_DESC_N] = disp.count(abi.HTTP_BAD_DESC)
    totals[abi.HTTP_HEADER_BYTES] = sum(m.header_len for m in found)
    totals[abi.HTTP_FIELDS_LINKED] = sum(len(m.fields) for m in found)
    if len(found) > (max_msgs or n) or (out_msgs is not None and len(found) > out_msgs) or \
            (out_fields is not None and len(recs) > out_fields) or \
            (want_text and text_cap is not None and len(out) > text_cap):
        totals[abi.HTTP_OVERFLOW] = 1
        return Result(totals, None, messages=found)
    return Result(totals, disp, msgs, recs, bytes(out) if want_text else b"", found)


def msgs_array(msgs: list) -> np.ndarray:
    """A model Result's messages as abi.HTTP_MSG_DTYPE."""
    out = np.zeros(len(msgs), abi.HTTP_MSG_DTYPE)
    for k, m in enumerate(msgs):
        out[k] = m
    return out


def fields_array(recs: list) -> np.ndarray:
    """A model Result's field records as abi.HTTP_FIELD_DTYPE."""
    out = np.zeros(len(recs), abi.HTTP_FIELD_DTYPE)
    for k, r in enumerate(recs):
        out[k] = r
    return out


# ------------------------------------------------------------------ the tables
def rows(msgs, fields, text) -> list[tuple]:
    """One row per field record: (source packet, kind, name_id, flags, name_len, value_len, the value's bytes where the
    call put them into the text, else b""). msgs: abi.HTTP_MSG_DTYPE; fields: abi.HTTP_FIELD_DTYPE; text: the call's
    text bytes."""
    text = bytes(text)
    out = []
    for r in fields:
        m = msgs[int(r["msg"])]
        pos = int(r["text_pos"])
        out.append((int(m["index"]), int(m["kind"]), int(r["name_id"]), int(r["flags"]), int(r["name_len"]),
                    int(r["value_len"]), text[pos:pos + int(r["text_len"])]))
    return out


def _esc(b: bytes) -> str:
    return b.decode("latin-1").encode("unicode_escape").decode("ascii")


def format_row(row: tuple) -> str:
    """A row as a line of text: the value with the bytes outside printable ASCII escaped."""
    pkt, kind, nid, fl, nl, vl, value = row
    return "\t".join([str(pkt), "response" if kind else "request", str(nid), str(fl), str(nl), str(vl), _esc(value)])


def analyze(msgs, fields, text, names=ANALYZE_NAMES) -> dict:
    """HttpAnalyzer's tables (Examples/HttpAnalyzer/HttpStatsCollector.h:434-494) from the records of a call whose spec
    had `names` (host, content-type among them), fields WANTED or ALL and text 3: messages and header bytes per kind,
    method counts and Host value counts of the requests, "<code> <message>" counts, Content-Type counts cut at the
    first ';' and the messages with a content length and their sum of the responses. Keys of the count tables are
    strings with the bytes outside printable ASCII escaped."""
    text = bytes(text)
    host, ctype = names.index("host"), names.index("content-type")
    first = {}  # (message, name_id) -> the value getFieldByName(name) has
    for r in fields:
        if int(r["flags"]) & abi.HTTP_FIRST and int(r["name_id"]) in (host, ctype):
            pos = int(r["text_pos"])
            first[(int(r["msg"]), int(r["name_id"]))] = text[pos:pos + int(r["text_len"])]
    out = {"requests": 0, "responses": 0, "request_header_bytes": 0, "response_header_bytes": 0, "methods": Counter(),
           "hosts": Counter(), "status": Counter(), "content_types": Counter(), "with_content_length": 0,
           "content_length_sum": 0}
    for j, m in enumerate(msgs):
        if int(m["kind"]) == abi.HTTP_REQUEST:
            out["requests"] += 1
            out["request_header_bytes"] += int(m["header_len"])
            k = int(m["method"])
            out["methods"][abi.HTTP_METHODS[k] if k < len(abi.HTTP_METHODS) else "unknown"] += 1
            if (j, host) in first:
                out["hosts"][_esc(first[(j, host)])] += 1
            continue
        out["responses"] += 1
        out["response_header_bytes"] += int(m["header_len"])
        if int(m["flags"]) & abi.HTTP_HAS_CONTENT_LENGTH:
            out["with_content_length"] += 1
            out["content_length_sum"] += int(m["content_length"])
        if (j, ctype) in first:
            out["content_types"][_esc(first[(j, ctype)].split(b";")[0])] += 1
        pos = int(m["text_pos"])
        out["status"][f"{int(m['status_code'])} {_esc(text[pos:pos + int(m['a_len'])])}"] += 1
    return {k: dict(v) if isinstance(v, Counter) else v for k, v in out.items()}
