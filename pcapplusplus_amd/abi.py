"""ctypes/numpy mirror of include/pcppx.h (the engine's C ABI) and the loader of libpcppx.so.

The loader fails loudly when the HIP engine library is missing: there is no CPU fallback in the
product path.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
ENGINE_SO = PKG_DIR / "libpcppx.so"

ABI_VERSION = 7
MAX_LAYERS = 16
MAX_CAPLEN = 65535
WINDOW_DEFAULT, WINDOW_DEEP, WINDOW_SHORT = 0, 1, 2  # pcppx_opts.window (PCPPX_WINDOW_*)
LAYOUT_FIXED, LAYOUT_PACKED, LAYOUT_DENSE = 0, 1, 2  # pcppx_opts.layout (PCPPX_LAYOUT_*); DENSE: host path
PACKED_MAX_LAYERS = 12
TILE = 64  # packets per tile of the PACKED layout

# error codes
OK, E_INVAL, E_NODEV, E_HIP, E_NOMEM, E_LINKTYPE = 0, -1, -2, -3, -4, -5

# summary flags
F_NEEDS_HOST_L7 = 0x0001
F_NEEDS_HOST_PROTO = 0x0002
F_DEPTH_OVERFLOW = 0x0004
F_OVERSIZE = 0x0008
F_IP_CSUM = 0x0010
F_IP_CSUM_OK = 0x0020
F_L4_CSUM = 0x0040
F_L4_CSUM_OK = 0x0080
F_TRAILER = 0x0100
F_BAD_DESC = 0x0200
F_L7_KNOWN = 0x0400
F_L7_HTTP = 0x0800
F_L7_SSL = 0x1000
F_L7_DNS = 0x2000
F_NEEDS_HOST = F_NEEDS_HOST_L7 | F_NEEDS_HOST_PROTO | F_OVERSIZE | F_BAD_DESC

# pcpp::LinkLayerType values used here (Packet++/header/RawPacket.h:24-178)
LINKTYPE_NULL = 0
LINKTYPE_ETHERNET = 1
LINKTYPE_DLT_RAW1 = 12
LINKTYPE_DLT_RAW2 = 14
LINKTYPE_RAW = 101
LINKTYPE_LINUX_SLL = 113
LINKTYPE_IPV4 = 228
LINKTYPE_IPV6 = 229

SUMMARY_DTYPE = np.dtype(
    [
        ("hash5", "<u4"),
        ("hash5_dir", "<u4"),
        ("hash2", "<u4"),
        ("flags", "<u2"),
        ("n_layers", "u1"),
        ("l4_layer", "u1"),
        ("proto_mask", "<u8"),
        ("ip_csum_calc", "<u2"),
        ("ip_csum_stored", "<u2"),
        ("l4_csum_calc", "<u2"),
        ("l4_csum_stored", "<u2"),
    ]
)
BRIEF_DTYPE = np.dtype(SUMMARY_DTYPE.descr[:6])  # pcppx_brief (ABI 7): the summary's first 16 bytes
LAYER_DTYPE = np.dtype(
    [("proto", "u1"), ("osi", "u1"), ("offset", "<u2"), ("hdr_len", "<u2"), ("data_len", "<u2")]
)
REASM_DTYPE = np.dtype(
    [("ip_key", "<u4"), ("frag_id", "<u4"), ("frag_offset", "<u2"), ("ip_status", "u1"), ("tcp_status", "u1"),
     ("tcp_payload", "<u4")]
)
TUPLE_DTYPE = np.dtype(
    [("src_ip", "u1", (16,)), ("dst_ip", "u1", (16,)), ("src_port", "<u2"), ("dst_port", "<u2"), ("ip_version", "u1"),
     ("ip_proto", "u1"), ("l4_proto", "u1"), ("has_5tuple", "u1"), ("hash5", "<u4"), ("flags", "<u2"),
     ("n_layers", "u1"), ("reserved", "u1")]
)
assert SUMMARY_DTYPE.itemsize == 32 and LAYER_DTYPE.itemsize == 8 and REASM_DTYPE.itemsize == 16
assert BRIEF_DTYPE.itemsize == 16
assert TUPLE_DTYPE.itemsize == 48

# pcppx_records.proto_stats words (PCPPX_PS_*): PacketStats::collectStats, Common.h:83-104
PROTO_STATS = 16
PROTO_STATS_FIELDS = ("packet_count", "eth_count", "arp_count", "ipv4_count", "ipv6_count", "tcp_count", "udp_count",
                      "http_count", "dns_count", "tls_count", "needs_host_count")

# pcppx_reasm_info status codes (low nibble) and flags
IPR_NON_IP, IPR_NON_FRAGMENT, IPR_MALFORMED, IPR_FRAGMENT, IPR_HOST = 0, 1, 2, 3, 15
IPR_F_FIRST, IPR_F_LAST, IPR_F_IPV6 = 0x10, 0x20, 0x40
TCPR_NON_IP, TCPR_NON_TCP, TCPR_NO_DATA, TCPR_DATA, TCPR_HOST = 0, 1, 2, 3, 15
TCPR_F_FIN, TCPR_F_SYN, TCPR_F_RST = 0x10, 0x20, 0x40


class Batch(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("offsets", C.c_void_p),
        ("caplens", C.c_void_p),
        ("data_len", C.c_uint64),
        ("n", C.c_uint32),
        ("linktype", C.c_uint16),
        ("reserved", C.c_uint16),
    ]


class Opts(C.Structure):
    _fields_ = [
        ("parse_until_family", C.c_uint32),
        ("parse_until_osi", C.c_uint8),
        ("want_checksums", C.c_uint8),
        ("max_layers", C.c_uint8),
        ("window", C.c_uint8),
        ("layout", C.c_uint8),
        ("reserved", C.c_uint8 * 3),
    ]


class Records(C.Structure):
    _fields_ = [("summary", C.c_void_p), ("layers", C.c_void_p), ("flow_keys", C.c_void_p), ("tuples", C.c_void_p),
                ("proto_stats", C.c_void_p), ("layout", C.c_uint8), ("reserved", C.c_uint8 * 7),
                ("brief", C.c_void_p), ("layers_written", C.c_uint64)]


class MatchSpec(C.Structure):
    """pcppx_match_spec: PacketMatchingEngine's criteria (PacketMatchingEngine.h:28-41)."""
    _fields_ = [("src_ip", C.c_uint32), ("dst_ip", C.c_uint32), ("src_port", C.c_uint16), ("dst_port", C.c_uint16),
                ("protocol", C.c_uint8), ("reserved", C.c_uint8 * 3)]


STATS_FIELDS = ("packet_count", "eth_count", "arp_count", "ipv4_count", "ipv6_count", "tcp_count", "udp_count",
                "http_count", "dns_count", "tls_count", "matched_tcp_flows", "matched_udp_flows", "matched_packets",
                "needs_host_count", "flow_table_full")


class PacketStats(C.Structure):
    """pcppx_packet_stats: PacketStats (Examples/DpdkExample-FilterTraffic/Common.h:57-142)."""
    _fields_ = [(f, C.c_uint64) for f in STATS_FIELDS]

    def as_dict(self) -> dict:
        return {f: int(getattr(self, f)) for f in STATS_FIELDS}


# pcppx_selection.totals words (PCPPX_SEL_*)
SEL_SELECTED_PACKETS, SEL_SELECTED_BYTES, SEL_WRITTEN_PACKETS, SEL_WRITTEN_BYTES, SEL_BAD_DESC = 0, 1, 2, 3, 4
SEL_TOTALS = 8
SEL_FIELDS = ("selected_packets", "selected_bytes", "written_packets", "written_bytes", "bad_desc")
FLAGS_OFFSET = SUMMARY_DTYPE.fields["flags"][1]  # the flags word's byte offset in a summary and in a brief
assert FLAGS_OFFSET == BRIEF_DTYPE.fields["flags"][1] == 12


class SelectSpec(C.Structure):
    """pcppx_select_spec: which packets pcppx_select_device gathers (a keep mask, or a test of the parse's flags)."""
    _fields_ = [("keep", C.c_void_p), ("flags", C.c_void_p), ("flags_stride", C.c_uint32), ("flags_any", C.c_uint16),
                ("invert", C.c_uint8), ("reserved", C.c_uint8), ("snaplen", C.c_uint32), ("reserved2", C.c_uint32)]


class Selection(C.Structure):
    """pcppx_selection: the packed output batch, the source index and the totals."""
    _fields_ = [("data", C.c_void_p), ("data_cap", C.c_uint64), ("offsets", C.c_void_p), ("caplens", C.c_void_p),
                ("index", C.c_void_p), ("max_packets", C.c_uint32), ("reserved", C.c_uint32), ("totals", C.c_void_p)]


def make_select_spec(keep=None, flags=None, flags_stride: int = 0, flags_any: int = 0, invert: bool = False,
                     snaplen: int = 0) -> SelectSpec:
    """keep: address of the n-byte mask, or flags: address of packet 0's 16-bit flags word (records + FLAGS_OFFSET)
    with flags_stride 32 (summary) / 16 (brief)."""
    return SelectSpec(keep, flags, flags_stride, flags_any, 1 if invert else 0, 0, snaplen, 0)


def totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(SEL_FIELDS)}


def select_reference(batch: Batch, spec: SelectSpec, out: Selection) -> None:
    """pcppx_select_reference: pcppx_select_device's contract in plain C++ over host pointers (no GPU). The structs
    hold addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_select_reference(C.byref(batch), C.byref(spec), C.byref(out)), "pcppx_select_reference")


# pcppx_steering.totals words (PCPPX_STEER_*)
STEER_STEERED_PACKETS, STEER_STEERED_BYTES, STEER_DROPPED, STEER_BAD_DESC, STEER_OVERFLOW = 0, 1, 2, 3, 4
STEER_TOTALS = 8
STEER_MAX_BUCKETS = 256
STEER_FIELDS = ("steered_packets", "steered_bytes", "dropped", "bad_desc", "overflow")


class SteerSpec(C.Structure):
    """pcppx_steer_spec: where pcppx_steer_device sends each packet (a bucket column, or a 32-bit key % n_buckets)."""
    _fields_ = [("bucket", C.c_void_p), ("key", C.c_void_p), ("key_stride", C.c_uint32), ("n_buckets", C.c_uint32),
                ("snaplen", C.c_uint32), ("reserved", C.c_uint32)]


class Steering(C.Structure):
    """pcppx_steering: the bucket-major packed output batch, the source index, the bucket bounds and the totals."""
    _fields_ = [("data", C.c_void_p), ("data_cap", C.c_uint64), ("offsets", C.c_void_p), ("caplens", C.c_void_p),
                ("index", C.c_void_p), ("bucket_first", C.c_void_p), ("bucket_pos", C.c_void_p),
                ("max_packets", C.c_uint32), ("reserved", C.c_uint32), ("totals", C.c_void_p)]


def make_steer_spec(bucket=None, key=None, key_stride: int = 4, n_buckets: int = 1, snaplen: int = 0) -> SteerSpec:
    """bucket: address of the n-byte bucket column, or key: address of packet 0's 32-bit key (records + the field's
    offset, e.g. SUMMARY_DTYPE.fields["hash5"][1]) with key_stride = the record size (4 for a plain u32 column)."""
    return SteerSpec(bucket, key, key_stride if key is not None else 0, n_buckets, snaplen, 0)


def steer_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(STEER_FIELDS)}


def steer_reference(batch: Batch, spec: SteerSpec, out: Steering) -> None:
    """pcppx_steer_reference: pcppx_steer_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_steer_reference(C.byref(batch), C.byref(spec), C.byref(out)), "pcppx_steer_reference")


# pcppx_defrag_*: the IPv4 fragment groups that are complete inside a batch (include/pcppx.h, defrag)
DEFRAG_MAX_FRAGS = 64
DEFRAG_PASS, DEFRAG_LEFT, DEFRAG_MERGED, DEFRAG_MERGED_LAST, DEFRAG_BAD_DESC = 0, 1, 2, 3, 4  # disposition values
(DEFRAG_OUT_PACKETS, DEFRAG_OUT_BYTES, DEFRAG_REASSEMBLED, DEFRAG_MERGED_FRAGS, DEFRAG_LEFT_FRAGS, DEFRAG_CANDIDATES,
 DEFRAG_BAD_DESC_N, DEFRAG_OVERFLOW) = range(8)  # pcppx_defragged.totals words
DEFRAG_TOTALS = 8
DEFRAG_FIELDS = ("out_packets", "out_bytes", "reassembled", "merged_frags", "left_frags", "candidates", "bad_desc",
                 "overflow")


class DefragSpec(C.Structure):
    """pcppx_defrag_spec: the room for candidates (0 = n) and whether the other packets are copied through."""
    _fields_ = [("max_fragments", C.c_uint32), ("passthrough", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class Defragged(C.Structure):
    """pcppx_defragged: the packed output batch, its per-packet columns, the per-source disposition and the totals."""
    _fields_ = [("data", C.c_void_p), ("data_cap", C.c_uint64), ("offsets", C.c_void_p), ("caplens", C.c_void_p),
                ("index", C.c_void_p), ("first", C.c_void_p), ("frags", C.c_void_p), ("disposition", C.c_void_p),
                ("max_packets", C.c_uint32), ("reserved", C.c_uint32), ("totals", C.c_void_p)]


def make_defrag_spec(passthrough: bool = True, max_fragments: int = 0) -> DefragSpec:
    return DefragSpec(max_fragments, 1 if passthrough else 0)


def defrag_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(DEFRAG_FIELDS)}


def defrag_reference(batch: Batch, records: Records, max_layers: int, info, spec: DefragSpec, out: Defragged) -> None:
    """pcppx_defrag_reference: pcppx_defrag_device's contract in plain C++ over host pointers (no GPU). info: the
    address of n pcppx_reasm_info; the structs hold addresses of host (numpy) arrays the caller keeps alive."""
    check(load_engine().pcppx_defrag_reference(C.byref(batch), C.byref(records), max_layers, info, C.byref(spec),
                                               C.byref(out)), "pcppx_defrag_reference")


# pcppx_defrag6_*: defrag for both families (include/pcppx.h, defrag6)
DEFRAG_FAM_V4, DEFRAG_FAM_V6 = 1, 2


class Defrag6Spec(C.Structure):
    """pcppx_defrag6_spec: pcppx_defrag_spec and the families (DEFRAG_FAM_* bits) whose groups are reassembled."""
    _fields_ = [("max_fragments", C.c_uint32), ("passthrough", C.c_uint8), ("families", C.c_uint8),
                ("reserved", C.c_uint8 * 2)]


def make_defrag6_spec(passthrough: bool = True, max_fragments: int = 0,
                      families: int = DEFRAG_FAM_V4 | DEFRAG_FAM_V6) -> Defrag6Spec:
    return Defrag6Spec(max_fragments, 1 if passthrough else 0, families)


def defrag6_reference(batch: Batch, records: Records, max_layers: int, info, spec: Defrag6Spec, out: Defragged) -> None:
    """pcppx_defrag6_reference: pcppx_defrag6_device's contract in plain C++ over host pointers (no GPU); the
    arguments are defrag_reference's."""
    check(load_engine().pcppx_defrag6_reference(C.byref(batch), C.byref(records), max_layers, info, C.byref(spec),
                                                C.byref(out)), "pcppx_defrag6_reference")


# pcppx_tcpstream_*: the TCP connection sides that are clean inside a batch (include/pcppx.h, tcpstream)
TCPS_F_SYN, TCPS_F_FIN, TCPS_F_RST, TCPS_F_OOO = 1, 2, 4, 8  # pcppx_tcpstream_rec.flags
TCPS_NOT_TCP, TCPS_HOST, TCPS_LEFT, TCPS_STREAM, TCPS_CONTROL, TCPS_BAD_DESC = range(6)  # disposition values
(TCPS_STREAMS, TCPS_BYTES, TCPS_SEGMENTS, TCPS_LEFT_N, TCPS_CANDIDATES, TCPS_HOST_N, TCPS_BAD_DESC_N,
 TCPS_OVERFLOW) = range(8)  # pcppx_tcpstreams.totals words
TCPS_TOTALS = 8
TCPS_NONE = 0xFFFFFFFF
TCPS_FIELDS = ("streams", "bytes", "segments", "left", "candidates", "host", "bad_desc", "overflow")
TCPSTREAM_DTYPE = np.dtype(
    [("pos", "<u8"), ("bytes", "<u4"), ("flow_key", "<u4"), ("first", "<u4"), ("segments", "<u4"), ("peer", "<u4"),
     ("side", "u1"), ("flags", "u1"), ("reserved", "u1", (2,))]
)
assert TCPSTREAM_DTYPE.itemsize == 32


class TcpStreamSpec(C.Structure):
    """pcppx_tcpstream_spec: the room for candidates (0 = n) and enableBaseBufferClearCondition."""
    _fields_ = [("max_segments", C.c_uint32), ("base_clear", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class TcpStreams(C.Structure):
    """pcppx_tcpstreams: the stream bytes, one record per clean side, the per-source columns and the totals."""
    _fields_ = [("data", C.c_void_p), ("data_cap", C.c_uint64), ("streams", C.c_void_p), ("disposition", C.c_void_p),
                ("seg_stream", C.c_void_p), ("seg_pos", C.c_void_p), ("max_streams", C.c_uint32),
                ("reserved", C.c_uint32), ("totals", C.c_void_p)]


def make_tcpstream_spec(base_clear: bool = True, max_segments: int = 0) -> TcpStreamSpec:
    return TcpStreamSpec(max_segments, 1 if base_clear else 0)


def tcpstream_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(TCPS_FIELDS)}


def tcpstream_reference(batch: Batch, records: Records, max_layers: int, info, spec: TcpStreamSpec,
                        out: TcpStreams) -> None:
    """pcppx_tcpstream_reference: pcppx_tcpstream_device's contract in plain C++ over host pointers (no GPU). info: the
    address of n pcppx_reasm_info; the structs hold addresses of host (numpy) arrays the caller keeps alive."""
    check(load_engine().pcppx_tcpstream_reference(C.byref(batch), C.byref(records), max_layers, info, C.byref(spec),
                                                  C.byref(out)), "pcppx_tcpstream_reference")


# pcppx_frag_*: the IPv4 packets of a batch split into fragments (include/pcppx.h, frag)
(FRAG_UNSELECTED, FRAG_NOT_V4, FRAG_ALREADY, FRAG_FITS, FRAG_DF, FRAG_SPLIT, FRAG_BAD_DESC) = range(7)  # disposition
(FRAG_OUT_PACKETS, FRAG_OUT_BYTES, FRAG_SPLIT_PACKETS, FRAG_FRAGMENTS, FRAG_COPIED, FRAG_UNDER_SIZE, FRAG_BAD_DESC_N,
 FRAG_OVERFLOW) = range(8)  # pcppx_fragmented.totals words
FRAG_TOTALS = 8
FRAG_FIELDS = ("out_packets", "out_bytes", "split_packets", "fragments", "copied", "under_size", "bad_desc", "overflow")


class FragSpec(C.Structure):
    """pcppx_frag_spec: the fragment size (or the MTU), the keep column, and what happens to the other packets."""
    _fields_ = [("keep", C.c_void_p), ("frag_size", C.c_uint32), ("mtu", C.c_uint32), ("copy_rest", C.c_uint8),
                ("honor_df", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class Fragmented(C.Structure):
    """pcppx_fragmented: the packed output batch, its per-packet columns, the per-source columns and the totals."""
    _fields_ = [("data", C.c_void_p), ("data_cap", C.c_uint64), ("offsets", C.c_void_p), ("caplens", C.c_void_p),
                ("index", C.c_void_p), ("frag_no", C.c_void_p), ("counts", C.c_void_p), ("disposition", C.c_void_p),
                ("max_packets", C.c_uint32), ("reserved", C.c_uint32), ("totals", C.c_void_p)]


def make_frag_spec(frag_size: int = 0, mtu: int = 0, keep=None, copy_rest: bool = True,
                   honor_df: bool = False) -> FragSpec:
    """frag_size (IPFragUtil's -s: a multiple of 8 in 8..65528) or mtu (68..65535), exactly one of them; keep: the
    address of the n-byte column of the packets to consider (None: all); copy_rest: IPFragUtil's -a."""
    return FragSpec(keep, frag_size, mtu, 1 if copy_rest else 0, 1 if honor_df else 0)


def frag_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(FRAG_FIELDS)}


def frag_reference(batch: Batch, records: Records, max_layers: int, spec: FragSpec, out: Fragmented) -> None:
    """pcppx_frag_reference: pcppx_frag_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_frag_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                             C.byref(out)), "pcppx_frag_reference")


# pcppx_frag6_*: frag for both families (include/pcppx.h, frag6)
FRAG_FAM_V4, FRAG_FAM_V6 = 1, 2
FRAG6_MAX_EXT = 16
FRAG_NOT_IP, FRAG_LEFT = FRAG_NOT_V4, 7  # two more disposition values


class Frag6Spec(C.Structure):
    """pcppx_frag6_spec: pcppx_frag_spec, the families (FRAG_FAM_* bits) whose packets are split, and the IPv6 fragment
    ids: a device column of n u32, or id_base + i."""
    _fields_ = [("keep", C.c_void_p), ("frag_size", C.c_uint32), ("mtu", C.c_uint32), ("copy_rest", C.c_uint8),
                ("honor_df", C.c_uint8), ("families", C.c_uint8), ("reserved", C.c_uint8 * 5), ("ids", C.c_void_p),
                ("id_base", C.c_uint32), ("reserved2", C.c_uint32)]


def make_frag6_spec(frag_size: int = 0, mtu: int = 0, families: int = FRAG_FAM_V4 | FRAG_FAM_V6, ids=None,
                    id_base: int = 0, keep=None, copy_rest: bool = True, honor_df: bool = False) -> Frag6Spec:
    """make_frag_spec's arguments; families: the FRAG_FAM_* bits; ids: the address of the n-entry u32 column of
    fragment ids (None: source packet i gets (id_base + i) mod 2^32)."""
    s = Frag6Spec(keep, frag_size, mtu, 1 if copy_rest else 0, 1 if honor_df else 0, families)
    s.ids, s.id_base = ids, id_base & 0xFFFFFFFF
    return s


def frag6_reference(batch: Batch, records: Records, max_layers: int, spec: Frag6Spec, out: Fragmented) -> None:
    """pcppx_frag6_reference: pcppx_frag6_device's contract in plain C++ over host pointers (no GPU); the arguments
    are frag_reference's."""
    check(load_engine().pcppx_frag6_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                              C.byref(out)), "pcppx_frag6_reference")


# pcppx_tlsfp_*: JA3 / JA3S fingerprints of the hello packets of a batch (include/pcppx.h, tlsfp)
TLSFP_NONE, TLSFP_CLIENT, TLSFP_SERVER, TLSFP_HOST, TLSFP_BAD_DESC = range(5)  # disposition; CLIENT / SERVER: rec.kind
(TLSFP_CLIENT_N, TLSFP_SERVER_N, TLSFP_TEXT_BYTES, TLSFP_HOST_N, TLSFP_BAD_DESC_N, TLSFP_CANDIDATES, _TLSFP_ZERO,
 TLSFP_OVERFLOW) = range(8)  # pcppx_tlsfps.totals words
TLSFP_TOTALS = 8
TLSFP_FIELDS = ("client_n", "server_n", "text_bytes", "host_n", "bad_desc", "candidates", "zero", "overflow")
TLSFP_REC_DTYPE = np.dtype(
    [("md5", "u1", (16,)), ("text_pos", "<u8"), ("text_len", "<u4"), ("index", "<u4"), ("msg_offset", "<u2"),
     ("kind", "u1"), ("reserved", "u1", (5,))]
)
assert TLSFP_REC_DTYPE.itemsize == 40


class TlsfpSpec(C.Structure):
    """pcppx_tlsfp_spec: the room for hello packets (0 = n) and which hellos are fingerprinted."""
    _fields_ = [("max_hellos", C.c_uint32), ("client", C.c_uint8), ("server", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class TlsfpRec(C.Structure):
    """pcppx_tlsfp_rec (TLSFP_REC_DTYPE is its numpy mirror)."""
    _fields_ = [("md5", C.c_uint8 * 16), ("text_pos", C.c_uint64), ("text_len", C.c_uint32), ("index", C.c_uint32),
                ("msg_offset", C.c_uint16), ("kind", C.c_uint8), ("reserved", C.c_uint8 * 5)]


class Tlsfps(C.Structure):
    """pcppx_tlsfps: the records, the texts back to back, the per-source disposition and the totals."""
    _fields_ = [("recs", C.c_void_p), ("text", C.c_void_p), ("text_cap", C.c_uint64), ("disposition", C.c_void_p),
                ("max_recs", C.c_uint32), ("reserved", C.c_uint32), ("totals", C.c_void_p)]


def make_tlsfp_spec(client: bool = True, server: bool = True, max_hellos: int = 0) -> TlsfpSpec:
    """client / server: the example's -t ch / sh / ch_sh."""
    return TlsfpSpec(max_hellos, 1 if client else 0, 1 if server else 0)


def tlsfp_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(TLSFP_FIELDS)}


def tlsfp_reference(batch: Batch, records: Records, max_layers: int, spec: TlsfpSpec, out: Tlsfps) -> None:
    """pcppx_tlsfp_reference: pcppx_tlsfp_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_tlsfp_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                              C.byref(out)), "pcppx_tlsfp_reference")


# pcppx_dns_*: DnsLayer's resource records of the DNS packets of a batch (include/pcppx.h, dns)
DNS_NONE, DNS_MSG, DNS_HOST, DNS_BAD_DESC = range(4)            # disposition
DNS_QUERY, DNS_ANSWER, DNS_AUTHORITY, DNS_ADDITIONAL = range(4)  # rr.section
DNS_COMPLETE, DNS_TRUNCATED, DNS_TOO_MANY = range(3)             # msg.status
(DNS_MSGS, DNS_RRS, DNS_NAME_BYTES, DNS_HOST_N, DNS_BAD_DESC_N, DNS_QA_LINKED, _DNS_ZERO,
 DNS_OVERFLOW) = range(8)  # pcppx_dns_out.totals words
DNS_TOTALS = 8
DNS_FIELDS = ("msgs", "rrs", "name_bytes", "host_n", "bad_desc", "qa_linked", "zero", "overflow")
DNS_MSG_DTYPE = np.dtype(
    [("first_rr", "<u8"), ("index", "<u4"), ("layer_offset", "<u2"), ("layer_len", "<u2"), ("id", "<u2"),
     ("flags", "<u2"), ("declared", "<u2", (4,)), ("linked", "<u2", (4,)), ("n_rr", "<u2"), ("adjust", "u1"),
     ("status", "u1")]
)
DNS_RR_DTYPE = np.dtype(
    [("name_pos", "<u8"), ("msg", "<u4"), ("ttl", "<u4"), ("offset", "<u2"), ("name_len", "<u2"), ("text_len", "<u2"),
     ("type", "<u2"), ("dns_class", "<u2"), ("data_len", "<u2"), ("data_offset", "<u2"), ("section", "u1"),
     ("reserved", "u1")]
)
assert DNS_MSG_DTYPE.itemsize == 40 and DNS_RR_DTYPE.itemsize == 32


class DnsSpec(C.Structure):
    """pcppx_dns_spec: the room for DNS packets (0 = n) and the sections whose resources get records."""
    _fields_ = [("max_msgs", C.c_uint32), ("sections", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class DnsMsg(C.Structure):
    """pcppx_dns_msg (DNS_MSG_DTYPE is its numpy mirror)."""
    _fields_ = [("first_rr", C.c_uint64), ("index", C.c_uint32), ("layer_offset", C.c_uint16),
                ("layer_len", C.c_uint16), ("id", C.c_uint16), ("flags", C.c_uint16), ("declared", C.c_uint16 * 4),
                ("linked", C.c_uint16 * 4), ("n_rr", C.c_uint16), ("adjust", C.c_uint8), ("status", C.c_uint8)]


class DnsRr(C.Structure):
    """pcppx_dns_rr (DNS_RR_DTYPE is its numpy mirror)."""
    _fields_ = [("name_pos", C.c_uint64), ("msg", C.c_uint32), ("ttl", C.c_uint32), ("offset", C.c_uint16),
                ("name_len", C.c_uint16), ("text_len", C.c_uint16), ("type", C.c_uint16), ("dns_class", C.c_uint16),
                ("data_len", C.c_uint16), ("data_offset", C.c_uint16), ("section", C.c_uint8), ("reserved", C.c_uint8)]


class DnsOut(C.Structure):
    """pcppx_dns_out: the messages, the resource records, the names back to back, the disposition and the totals."""
    _fields_ = [("msgs", C.c_void_p), ("rrs", C.c_void_p), ("names", C.c_void_p), ("names_cap", C.c_uint64),
                ("disposition", C.c_void_p), ("max_msgs", C.c_uint32), ("max_rrs", C.c_uint32),
                ("totals", C.c_void_p)]


def make_dns_spec(sections: int = 15, max_msgs: int = 0) -> DnsSpec:
    """sections: bit 0 queries, 1 answers, 2 authorities, 3 additionals."""
    return DnsSpec(max_msgs, sections)


def dns_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(DNS_FIELDS)}


def dns_reference(batch: Batch, records: Records, max_layers: int, spec: DnsSpec, out: DnsOut) -> None:
    """pcppx_dns_reference: pcppx_dns_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_dns_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                            C.byref(out)), "pcppx_dns_reference")


# pcppx_http_*: the first line and the header fields of the HTTP packets of a batch (include/pcppx.h, http)
HTTP_NONE, HTTP_MSG, HTTP_HOST, HTTP_BAD_DESC = range(4)  # disposition
HTTP_REQUEST, HTTP_RESPONSE = 0, 1                        # msg.kind
HTTP_KIND_REQUESTS, HTTP_KIND_RESPONSES = 1, 2            # spec.kinds bits
HTTP_FIELDS_NONE, HTTP_FIELDS_WANTED, HTTP_FIELDS_ALL = range(3)  # spec.fields
HTTP_TEXT_FIRST_LINE, HTTP_TEXT_VALUES = 1, 2             # spec.text bits
HTTP_METHODS = ("GET", "HEAD", "POST", "PUT", "DELETE", "TRACE", "OPTIONS", "CONNECT", "PATCH")  # msg.method 0..8
HTTP_METHOD_UNKNOWN = 9
HTTP_VERSIONS = ("0.9", "1.0", "1.1")                     # msg.version 0..2
HTTP_VERSION_UNKNOWN = 3
HTTP_FIRST_LINE_COMPLETE, HTTP_HEADER_COMPLETE, HTTP_HAS_CONTENT_LENGTH, HTTP_CONTENT_LENGTH_RANGE = 1, 2, 4, 8
HTTP_HAS_VALUE, HTTP_FIRST = 1, 2                         # field.flags
HTTP_NO_NAME = 0xFF
HTTP_MAX_NAMES, HTTP_NAME_MAX = 8, 32
(HTTP_MSGS, HTTP_REQUESTS, HTTP_RESPONSES, HTTP_FIELDS, HTTP_TEXT_BYTES, HTTP_HOST_N, HTTP_BAD_DESC_N,
 HTTP_HEADER_BYTES, HTTP_FIELDS_LINKED, _HTTP_ZERO0, _HTTP_ZERO1, HTTP_OVERFLOW) = range(12)  # pcppx_http_out.totals
HTTP_TOTALS = 12
HTTP_TOTAL_NAMES = ("msgs", "requests", "responses", "fields", "text_bytes", "host_n", "bad_desc", "header_bytes",
                    "fields_linked", "zero0", "zero1", "overflow")
HTTP_MSG_DTYPE = np.dtype(
    [("first_field", "<u8"), ("text_pos", "<u8"), ("index", "<u4"), ("content_length", "<i4"), ("layer_offset", "<u2"),
     ("layer_len", "<u2"), ("header_len", "<u2"), ("first_line_len", "<u2"), ("n_fields", "<u2"), ("n_rec", "<u2"),
     ("a_offset", "<u2"), ("a_len", "<u2"), ("status_code", "<u2"), ("text_len", "<u2"), ("kind", "u1"),
     ("method", "u1"), ("version", "u1"), ("flags", "u1")]
)
HTTP_FIELD_DTYPE = np.dtype(
    [("text_pos", "<u8"), ("msg", "<u4"), ("name_offset", "<u2"), ("name_len", "<u2"), ("value_offset", "<u2"),
     ("value_len", "<u2"), ("text_len", "<u2"), ("name_id", "u1"), ("flags", "u1")]
)
assert HTTP_MSG_DTYPE.itemsize == 48 and HTTP_FIELD_DTYPE.itemsize == 24


class HttpSpec(C.Structure):
    """pcppx_http_spec: the room for HTTP packets (0 = n), the kinds, which fields get records, which bytes go to the
    text, and the wanted names in lower case."""
    _fields_ = [("max_msgs", C.c_uint32), ("kinds", C.c_uint8), ("fields", C.c_uint8), ("text", C.c_uint8),
                ("n_names", C.c_uint8), ("name_len", C.c_uint8 * 8), ("names", (C.c_char * 32) * 8)]


class HttpMsg(C.Structure):
    """pcppx_http_msg (HTTP_MSG_DTYPE is its numpy mirror)."""
    _fields_ = [("first_field", C.c_uint64), ("text_pos", C.c_uint64), ("index", C.c_uint32),
                ("content_length", C.c_int32), ("layer_offset", C.c_uint16), ("layer_len", C.c_uint16),
                ("header_len", C.c_uint16), ("first_line_len", C.c_uint16), ("n_fields", C.c_uint16),
                ("n_rec", C.c_uint16), ("a_offset", C.c_uint16), ("a_len", C.c_uint16), ("status_code", C.c_uint16),
                ("text_len", C.c_uint16), ("kind", C.c_uint8), ("method", C.c_uint8), ("version", C.c_uint8),
                ("flags", C.c_uint8)]


class HttpField(C.Structure):
    """pcppx_http_field (HTTP_FIELD_DTYPE is its numpy mirror)."""
    _fields_ = [("text_pos", C.c_uint64), ("msg", C.c_uint32), ("name_offset", C.c_uint16), ("name_len", C.c_uint16),
                ("value_offset", C.c_uint16), ("value_len", C.c_uint16), ("text_len", C.c_uint16),
                ("name_id", C.c_uint8), ("flags", C.c_uint8)]


class HttpOut(C.Structure):
    """pcppx_http_out: the messages, the field records, the text back to back, the disposition and the totals."""
    _fields_ = [("msgs", C.c_void_p), ("fields", C.c_void_p), ("text", C.c_void_p), ("text_cap", C.c_uint64),
                ("disposition", C.c_void_p), ("max_msgs", C.c_uint32), ("max_fields", C.c_uint32),
                ("totals", C.c_void_p)]


def make_http_spec(names=(), fields: int = HTTP_FIELDS_WANTED, text: int = 3, kinds: int = 3,
                   max_msgs: int = 0) -> HttpSpec:
    """names: up to 8 field names of 1..32 bytes (str or bytes), lower case; the call refuses anything else."""
    s = HttpSpec(max_msgs, kinds, fields, text, len(names))
    for k, nm in enumerate(names[:HTTP_MAX_NAMES]):
        raw = nm.encode("latin-1") if isinstance(nm, str) else bytes(nm)
        s.name_len[k] = min(len(raw), 255)
        C.memmove(C.addressof(s.names[k]), raw[:HTTP_NAME_MAX], min(len(raw), HTTP_NAME_MAX))
    return s


def http_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(HTTP_TOTAL_NAMES)}


def http_reference(batch: Batch, records: Records, max_layers: int, spec: HttpSpec, out: HttpOut) -> None:
    """pcppx_http_reference: pcppx_http_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_http_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                             C.byref(out)), "pcppx_http_reference")


# pcppx_ssl_*: the SSL/TLS records, the hellos and the SNI of the SSL packets of a batch (include/pcppx.h, ssl)
SSL_NONE, SSL_MSG, SSL_HOST, SSL_BAD_DESC = range(4)  # disposition
SSL_CLIENT, SSL_SERVER = 1, 2                         # hello.kind
SSL_KIND_CLIENT, SSL_KIND_SERVER = 1, 2               # spec.kinds bits
SSL_NO_TCP = 1                                        # msg.flags
SSL_HAS_SNI, SSL_SNI_TRUNCATED, SSL_SNI_MALFORMED, SSL_HAS_CIPHER = 1, 2, 4, 8  # hello.flags
(SSL_MSGS, SSL_HELLOS, SSL_CLIENT_HELLOS, SSL_SERVER_HELLOS, SSL_NAME_BYTES, SSL_HOST_N, SSL_BAD_DESC_N,
 SSL_PAYLOAD_BYTES, SSL_ALERT_PKTS, SSL_APPDATA_PKTS, _SSL_ZERO, SSL_OVERFLOW) = range(12)  # pcppx_ssl_out.totals
SSL_TOTALS = 12
SSL_TOTAL_NAMES = ("msgs", "hellos", "client_hellos", "server_hellos", "name_bytes", "host_n", "bad_desc",
                   "payload_bytes", "alert_pkts", "appdata_pkts", "zero", "overflow")
SSL_MSG_DTYPE = np.dtype(
    [("first_hello", "<u8"), ("index", "<u4"), ("name_bytes", "<u4"), ("layer_offset", "<u2"), ("payload_len", "<u2"),
     ("src_port", "<u2"), ("dst_port", "<u2"), ("ssl_port", "<u2"), ("n_handshake", "u1"), ("n_ccs", "u1"),
     ("n_alert", "u1"), ("n_appdata", "u1"), ("n_hellos", "u1"), ("flags", "u1")]
)
SSL_HELLO_DTYPE = np.dtype(
    [("name_pos", "<u8"), ("msg", "<u4"), ("msg_offset", "<u2"), ("name_len", "<u2"), ("version", "<u2"),
     ("header_version", "<u2"), ("cipher", "<u2"), ("n_ciphers", "<u2"), ("n_ext", "<u2"), ("kind", "u1"),
     ("layer", "u1"), ("session_id_len", "u1"), ("flags", "u1"), ("reserved", "u1", (2,))]
)
assert SSL_MSG_DTYPE.itemsize == 32 and SSL_HELLO_DTYPE.itemsize == 32


class SslSpec(C.Structure):
    """pcppx_ssl_spec: the room for SSL packets (0 = n) and the hello kinds that get records."""
    _fields_ = [("max_msgs", C.c_uint32), ("kinds", C.c_uint8), ("reserved", C.c_uint8 * 3)]


class SslMsg(C.Structure):
    """pcppx_ssl_msg (SSL_MSG_DTYPE is its numpy mirror)."""
    _fields_ = [("first_hello", C.c_uint64), ("index", C.c_uint32), ("name_bytes", C.c_uint32),
                ("layer_offset", C.c_uint16), ("payload_len", C.c_uint16), ("src_port", C.c_uint16),
                ("dst_port", C.c_uint16), ("ssl_port", C.c_uint16), ("n_handshake", C.c_uint8), ("n_ccs", C.c_uint8),
                ("n_alert", C.c_uint8), ("n_appdata", C.c_uint8), ("n_hellos", C.c_uint8), ("flags", C.c_uint8)]


class SslHello(C.Structure):
    """pcppx_ssl_hello (SSL_HELLO_DTYPE is its numpy mirror)."""
    _fields_ = [("name_pos", C.c_uint64), ("msg", C.c_uint32), ("msg_offset", C.c_uint16), ("name_len", C.c_uint16),
                ("version", C.c_uint16), ("header_version", C.c_uint16), ("cipher", C.c_uint16),
                ("n_ciphers", C.c_uint16), ("n_ext", C.c_uint16), ("kind", C.c_uint8), ("layer", C.c_uint8),
                ("session_id_len", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8 * 2)]


class SslOut(C.Structure):
    """pcppx_ssl_out: the messages, the hello records, the host names back to back, the disposition and the totals."""
    _fields_ = [("msgs", C.c_void_p), ("hellos", C.c_void_p), ("names", C.c_void_p), ("names_cap", C.c_uint64),
                ("disposition", C.c_void_p), ("max_msgs", C.c_uint32), ("max_hellos", C.c_uint32),
                ("totals", C.c_void_p)]


def make_ssl_spec(kinds: int = 3, max_msgs: int = 0) -> SslSpec:
    return SslSpec(max_msgs, kinds)


def ssl_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(SSL_TOTAL_NAMES)}


def ssl_reference(batch: Batch, records: Records, max_layers: int, spec: SslSpec, out: SslOut) -> None:
    """pcppx_ssl_reference: pcppx_ssl_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_ssl_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                            C.byref(out)), "pcppx_ssl_reference")


# pcppx_sip_*: the SIP messages, their header fields and their SDP bodies of a batch (include/pcppx.h, sip)
SIP_NONE, SIP_MSG, SIP_HOST, SIP_BAD_DESC = range(4)  # disposition
SIP_REQUEST, SIP_RESPONSE = 0, 1                      # msg.kind
SIP_VIA_PORT, SIP_VIA_HEURISTIC = 0, 1                # msg.via
SIP_METHODS = ("INVITE", "ACK", "BYE", "CANCEL", "REGISTER", "PRACK", "OPTIONS", "SUBSCRIBE", "NOTIFY", "PUBLISH",
               "INFO", "REFER", "MESSAGE", "UPDATE")  # msg.method 0..13
SIP_METHOD_UNKNOWN = 14
(SIP_FIRST_LINE_COMPLETE, SIP_HEADER_COMPLETE, SIP_HAS_CONTENT_LENGTH, SIP_CONTENT_LENGTH_RANGE, SIP_VERSION_KNOWN,
 SIP_HAS_SDP, SIP_CARRIER_TCP) = 1, 2, 4, 8, 16, 32, 64  # msg.flags
SIP_SDP_HAS_OWNER, SIP_SDP_HAS_AUDIO, SIP_SDP_HAS_VIDEO = 1, 2, 4  # sdp.flags
(SIP_MSGS, SIP_REQUESTS, SIP_RESPONSES, SIP_FIELDS, SIP_TEXT_BYTES, SIP_HOST_N, SIP_BAD_DESC_N, SIP_HEADER_BYTES,
 SIP_FIELDS_LINKED, SIP_SDPS, SIP_BY_HEURISTIC, SIP_OVERFLOW) = range(12)  # pcppx_sip_out.totals
SIP_TOTALS = 12
SIP_TOTAL_NAMES = ("msgs", "requests", "responses", "fields", "text_bytes", "host_n", "bad_desc", "header_bytes",
                   "fields_linked", "sdps", "by_heuristic", "overflow")
SIP_MSG_DTYPE = np.dtype(
    [("first_field", "<u8"), ("text_pos", "<u8"), ("index", "<u4"), ("content_length", "<i4"), ("layer_offset", "<u2"),
     ("layer_len", "<u2"), ("header_len", "<u2"), ("first_line_len", "<u2"), ("n_fields", "<u2"), ("n_rec", "<u2"),
     ("a_offset", "<u2"), ("a_len", "<u2"), ("status_code", "<u2"), ("text_len", "<u2"), ("kind", "u1"),
     ("method", "u1"), ("via", "u1"), ("flags", "u1")]
)
SIP_FIELD_DTYPE = HTTP_FIELD_DTYPE  # pcppx_sip_field is pcppx_http_field
SIP_SDP_DTYPE = np.dtype(
    [("msg", "<u4"), ("index", "<u4"), ("offset", "<u2"), ("len", "<u2"), ("n_fields", "<u2"), ("audio_port", "<u2"),
     ("video_port", "<u2"), ("flags", "u1"), ("reserved0", "u1"), ("owner_ipv4", "u1", (4,)), ("reserved", "u1", (8,))]
)
assert SIP_MSG_DTYPE.itemsize == 48 and SIP_SDP_DTYPE.itemsize == 32

SipSpec = HttpSpec    # pcppx_sip_spec is pcppx_http_spec
SipField = HttpField  # pcppx_sip_field is pcppx_http_field


class SipMsg(C.Structure):
    """pcppx_sip_msg (SIP_MSG_DTYPE is its numpy mirror)."""
    _fields_ = [("first_field", C.c_uint64), ("text_pos", C.c_uint64), ("index", C.c_uint32),
                ("content_length", C.c_int32), ("layer_offset", C.c_uint16), ("layer_len", C.c_uint16),
                ("header_len", C.c_uint16), ("first_line_len", C.c_uint16), ("n_fields", C.c_uint16),
                ("n_rec", C.c_uint16), ("a_offset", C.c_uint16), ("a_len", C.c_uint16), ("status_code", C.c_uint16),
                ("text_len", C.c_uint16), ("kind", C.c_uint8), ("method", C.c_uint8), ("via", C.c_uint8),
                ("flags", C.c_uint8)]


class SipSdp(C.Structure):
    """pcppx_sip_sdp (SIP_SDP_DTYPE is its numpy mirror)."""
    _fields_ = [("msg", C.c_uint32), ("index", C.c_uint32), ("offset", C.c_uint16), ("len", C.c_uint16),
                ("n_fields", C.c_uint16), ("audio_port", C.c_uint16), ("video_port", C.c_uint16),
                ("flags", C.c_uint8), ("reserved0", C.c_uint8), ("owner_ipv4", C.c_uint8 * 4),
                ("reserved", C.c_uint8 * 8)]


class SipOut(C.Structure):
    """pcppx_sip_out: the messages, the field records, the SDP records, the text back to back, the disposition and the
    totals."""
    _fields_ = [("msgs", C.c_void_p), ("fields", C.c_void_p), ("sdps", C.c_void_p), ("text", C.c_void_p),
                ("text_cap", C.c_uint64), ("disposition", C.c_void_p), ("max_msgs", C.c_uint32),
                ("max_fields", C.c_uint32), ("max_sdps", C.c_uint32), ("reserved", C.c_uint32),
                ("totals", C.c_void_p)]


SIP_CALL_NAMES = ("call-id", "from", "to", "cseq")  # what a VoIP monitor keys a dialog by


def make_sip_spec(names=SIP_CALL_NAMES, fields: int = HTTP_FIELDS_WANTED, text: int = 3, kinds: int = 3,
                  max_msgs: int = 0) -> HttpSpec:
    """names: up to 8 field names of 1..32 bytes (str or bytes), lower case; the call refuses anything else."""
    return make_http_spec(names, fields, text, kinds, max_msgs)


def sip_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(SIP_TOTAL_NAMES)}


def sip_reference(batch: Batch, records: Records, max_layers: int, spec: HttpSpec, out: SipOut) -> None:
    """pcppx_sip_reference: pcppx_sip_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_sip_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                            C.byref(out)), "pcppx_sip_reference")


# pcppx_dhcp_*: the DHCP and DHCPv6 messages and their options of a batch (include/pcppx.h, dhcp)
DHCP_NONE, DHCP_MSG, DHCP_HOST, DHCP_BAD_DESC = range(4)  # disposition
DHCP_V4, DHCP_V6 = 1, 2                                   # spec.families bits
DHCP_OPTIONS_NONE, DHCP_OPTIONS_WANTED, DHCP_OPTIONS_ALL = 0, 1, 2  # spec.options
DHCP_MAX_CODES6 = 16
(DHCP_HAS_MSG_TYPE, DHCP_HAS_MAC, DHCP_MAGIC_OK, DHCP_HAS_LEASE_TIME, DHCP_HAS_SERVER_ID,
 DHCP_REPLY) = 1, 2, 4, 8, 16, 32  # msg.flags
(DHCP_MSGS, DHCP_V4_N, DHCP_V6_N, DHCP_OPTIONS, DHCP_VALUE_BYTES, DHCP_HOST_N, DHCP_BAD_DESC_N, DHCP_OPTIONS_LINKED,
 DHCP_REPLIES, DHCP_OVERFLOW) = range(10)  # pcppx_dhcp_out.totals
DHCP_TOTALS = 10
DHCP_TOTAL_NAMES = ("msgs", "v4", "v6", "options", "value_bytes", "host_n", "bad_desc", "options_linked", "replies",
                    "overflow")
DHCP_MSG_TYPES = ("UNKNOWN", "DISCOVER", "OFFER", "REQUEST", "DECLINE", "ACK", "NAK", "RELEASE", "INFORM")  # DHCPv4
DHCP_MSG_DTYPE = np.dtype(
    [("first_option", "<u8"), ("value_pos", "<u8"), ("index", "<u4"), ("xid", "<u4"), ("lease_time", "<u4"),
     ("layer_offset", "<u2"), ("layer_len", "<u2"), ("n_options", "<u2"), ("n_rec", "<u2"), ("value_len", "<u2"),
     ("options_len", "<u2"), ("secs", "<u2"), ("bootp_flags", "<u2"), ("family", "u1"), ("msg_type", "u1"),
     ("flags", "u1"), ("op", "u1"), ("htype", "u1"), ("hlen", "u1"), ("hops", "u1"), ("reserved0", "u1"),
     ("ciaddr", "u1", (4,)), ("yiaddr", "u1", (4,)), ("siaddr", "u1", (4,)), ("giaddr", "u1", (4,)),
     ("server_id", "u1", (4,)), ("client_mac", "u1", (6,)), ("reserved", "u1", (2,))]
)
DHCP_OPTION_DTYPE = np.dtype(
    [("msg", "<u4"), ("code", "<u2"), ("len", "<u2"), ("offset", "<u2"), ("ordinal", "<u2"), ("value_rel", "<u2"),
     ("reserved", "<u2")]
)
assert DHCP_MSG_DTYPE.itemsize == 80 and DHCP_OPTION_DTYPE.itemsize == 16


class DhcpSpec(C.Structure):
    """pcppx_dhcp_spec: the room for messages (0 = n), the families, which options get records and whether their
    values are copied, the wanted DHCPv4 codes as a 256-bit mask and the wanted DHCPv6 codes in ascending order."""
    _fields_ = [("max_msgs", C.c_uint32), ("families", C.c_uint8), ("options", C.c_uint8), ("values", C.c_uint8),
                ("n_codes6", C.c_uint8), ("want4", C.c_uint32 * 8), ("want6", C.c_uint16 * 16)]


class DhcpOption(C.Structure):
    """pcppx_dhcp_option (DHCP_OPTION_DTYPE is its numpy mirror)."""
    _fields_ = [("msg", C.c_uint32), ("code", C.c_uint16), ("len", C.c_uint16), ("offset", C.c_uint16),
                ("ordinal", C.c_uint16), ("value_rel", C.c_uint16), ("reserved", C.c_uint16)]


class DhcpMsg(C.Structure):
    """pcppx_dhcp_msg (DHCP_MSG_DTYPE is its numpy mirror)."""
    _fields_ = [("first_option", C.c_uint64), ("value_pos", C.c_uint64), ("index", C.c_uint32), ("xid", C.c_uint32),
                ("lease_time", C.c_uint32), ("layer_offset", C.c_uint16), ("layer_len", C.c_uint16),
                ("n_options", C.c_uint16), ("n_rec", C.c_uint16), ("value_len", C.c_uint16),
                ("options_len", C.c_uint16), ("secs", C.c_uint16), ("bootp_flags", C.c_uint16), ("family", C.c_uint8),
                ("msg_type", C.c_uint8), ("flags", C.c_uint8), ("op", C.c_uint8), ("htype", C.c_uint8),
                ("hlen", C.c_uint8), ("hops", C.c_uint8), ("reserved0", C.c_uint8), ("ciaddr", C.c_uint8 * 4),
                ("yiaddr", C.c_uint8 * 4), ("siaddr", C.c_uint8 * 4), ("giaddr", C.c_uint8 * 4),
                ("server_id", C.c_uint8 * 4), ("client_mac", C.c_uint8 * 6), ("reserved", C.c_uint8 * 2)]


class DhcpOut(C.Structure):
    """pcppx_dhcp_out: the messages, the option records, the values back to back, the disposition and the totals."""
    _fields_ = [("msgs", C.c_void_p), ("options", C.c_void_p), ("values", C.c_void_p), ("values_cap", C.c_uint64),
                ("disposition", C.c_void_p), ("max_msgs", C.c_uint32), ("max_options", C.c_uint32),
                ("reserved", C.c_uint64), ("totals", C.c_void_p)]


DHCP_ASSET_CODES4 = (12, 50, 51, 53, 54, 55, 60, 61)  # host name, requested address, lease, type, server, lists, ids
DHCP_ASSET_CODES6 = (1, 2, 3, 39)                     # client id, server id, IA_NA, client FQDN


def make_dhcp_spec(codes4=DHCP_ASSET_CODES4, codes6=DHCP_ASSET_CODES6, options: int = DHCP_OPTIONS_WANTED,
                   values: int = 1, families: int = 3, max_msgs: int = 0) -> DhcpSpec:
    """codes4: wanted DHCPv4 codes 0..255; codes6: up to 16 wanted DHCPv6 codes, written as given (the call refuses a
    list that is not strictly ascending)."""
    s = DhcpSpec(max_msgs, families, options, values, min(len(codes6), 255))
    for c in codes4:
        s.want4[(c & 255) >> 5] |= 1 << (c & 31)
    for k, c in enumerate(codes6[:DHCP_MAX_CODES6]):
        s.want6[k] = c
    return s


def dhcp_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(DHCP_TOTAL_NAMES)}


def dhcp_reference(batch: Batch, records: Records, max_layers: int, spec: DhcpSpec, out: DhcpOut) -> None:
    """pcppx_dhcp_reference: pcppx_dhcp_device's contract in plain C++ over host pointers (no GPU). The structs hold
    addresses of host (numpy) arrays the caller keeps alive; out's arrays and totals are filled in place."""
    check(load_engine().pcppx_dhcp_reference(C.byref(batch), C.byref(records), max_layers, C.byref(spec),
                                             C.byref(out)), "pcppx_dhcp_reference")


# pcppx_bpf_*: classic BPF programs over a batch (include/pcppx.h, bpf)
BPF_MAX_INSNS, BPF_MAX_PROGRAMS, BPF_MEMWORDS = 4096, 16, 16
BPF_MATCHED, BPF_BAD_DESC = 0, 1  # pcppx_bpf_verdicts.totals words (PCPPX_BPF_*)
BPF_TOTALS = 8
BPF_FIELDS = ("matched", "bad_desc")
BPF_NO_BUCKET = 0xFF
BPF_INSN_DTYPE = np.dtype([("code", "<u2"), ("jt", "u1"), ("jf", "u1"), ("k", "<u4")])  # pcppx_bpf_insn
assert BPF_INSN_DTYPE.itemsize == 8


class BpfInsn(C.Structure):
    """pcppx_bpf_insn: struct bpf_insn / sock_filter."""
    _fields_ = [("code", C.c_uint16), ("jt", C.c_uint8), ("jf", C.c_uint8), ("k", C.c_uint32)]


class BpfProg(C.Structure):
    """pcppx_bpf_prog: one program in host memory."""
    _fields_ = [("insns", C.c_void_p), ("n_insns", C.c_uint32), ("reserved", C.c_uint32)]


class BpfVerdicts(C.Structure):
    """pcppx_bpf_verdicts: the per-packet columns (each may be None) and the totals."""
    _fields_ = [("matched", C.c_void_p), ("bucket", C.c_void_p), ("ret", C.c_void_p), ("totals", C.c_void_p)]


def bpf_program(insns) -> np.ndarray:
    """A program as a contiguous BPF_INSN_DTYPE array: from such an array, or from (code, jt, jf, k) rows."""
    if isinstance(insns, np.ndarray) and insns.dtype == BPF_INSN_DTYPE:
        return np.ascontiguousarray(insns)
    return np.array([tuple(int(x) for x in row) for row in insns], dtype=BPF_INSN_DTYPE)


def make_bpf_progs(programs):
    """(pcppx_bpf_prog array, the instruction arrays it points to: keep them alive) for a list of programs."""
    arrays = [bpf_program(p) for p in programs]
    progs = (BpfProg * max(len(arrays), 1))()
    for q, a in enumerate(arrays):
        progs[q] = BpfProg(a.ctypes.data, len(a), 0)
    return progs, arrays


def bpf_validate(insns) -> bool:
    """pcppx_bpf_validate: whether pcppx_bpf_load would take the program (host only)."""
    a = bpf_program(insns)
    return load_engine().pcppx_bpf_validate(a.ctypes.data if len(a) else None, len(a)) == OK


def bpf_totals_dict(totals) -> dict:
    return {f: int(totals[k]) for k, f in enumerate(BPF_FIELDS)}


def bpf_reference(programs, batch: Batch, frame_lens, out: BpfVerdicts) -> None:
    """pcppx_bpf_reference: pcppx_bpf_device's contract in plain C++ over host pointers (no GPU). frame_lens: the
    address of n u32, or None; out's arrays and totals are filled in place."""
    progs, keep = make_bpf_progs(programs)
    check(load_engine().pcppx_bpf_reference(progs, len(keep), C.byref(batch), frame_lens, C.byref(out)),
          "pcppx_bpf_reference")


def ipv4_to_int(dotted: str) -> int:
    """IPv4Address::toInt(): the address bytes in memory order read as a little-endian u32."""
    b = bytes(int(x) for x in dotted.split("."))
    return int.from_bytes(b, "little")


def make_opts(parse_until_family: int = 0, parse_until_osi: int = 8, want_checksums: bool = True,
              max_layers: int = MAX_LAYERS, window: int = 0, layout: int = LAYOUT_FIXED) -> Opts:
    """pcpp::PacketParseOptions defaults (Packet++/header/Packet.h:17-37) + output selection; window:
    WINDOW_DEFAULT / WINDOW_DEEP / WINDOW_SHORT (the header window the parse gathers: a speed choice, records
    identical; DEEP: two rounds for checksum launches, SHORT: one 96-B round for parse-only launches); layout: LAYOUT_FIXED /
    LAYOUT_PACKED (the layer entries, bit for bit the same; unpack_layers)."""
    if not 0 <= max_layers <= MAX_LAYERS:
        raise ValueError(f"max_layers must be in [0, {MAX_LAYERS}]")
    if window not in (WINDOW_DEFAULT, WINDOW_DEEP, WINDOW_SHORT):
        raise ValueError("window must be WINDOW_DEFAULT, WINDOW_DEEP or WINDOW_SHORT")
    if layout not in (LAYOUT_FIXED, LAYOUT_PACKED, LAYOUT_DENSE) or \
            (layout == LAYOUT_PACKED and max_layers > PACKED_MAX_LAYERS):
        raise ValueError(f"layout must be LAYOUT_FIXED, LAYOUT_DENSE (host path), or LAYOUT_PACKED with max_layers <= "
                         f"{PACKED_MAX_LAYERS}")
    o = Opts(parse_until_family, parse_until_osi, 1 if want_checksums else 0, max_layers, window)
    o.layout = layout
    return o


def packed_positions(n_layers: np.ndarray, max_layers: int) -> np.ndarray:
    """Start entry of every packet's chain in a PACKED layer array (include/pcppx.h PCPPX_LAYOUT_PACKED): the tile's
    base 64 * t * max_layers plus the chains of the packets before it in its 64-packet tile."""
    cnt = np.minimum(n_layers.astype(np.int64), max_layers)
    n = len(cnt)
    tile = np.arange(n) // TILE
    csum = np.cumsum(cnt) - cnt  # exclusive prefix over the whole batch
    first = tile * TILE
    return tile * TILE * max_layers + csum - csum[first] if n else csum


def unpack_layers(summary: np.ndarray, packed: np.ndarray, max_layers: int) -> np.ndarray:
    """PACKED layer entries -> the FIXED [n, max_layers] array (entries past a chain zero)."""
    n = len(summary)
    out = np.zeros((n, max_layers), dtype=LAYER_DTYPE)
    if n == 0 or max_layers == 0:
        return out
    cnt = np.minimum(summary["n_layers"].astype(np.int64), max_layers)
    start = packed_positions(summary["n_layers"], max_layers)
    flat = packed.reshape(-1)
    for k in range(max_layers):
        m = cnt > k
        out[m, k] = flat[start[m] + k]
    return out


def dense_positions(n_layers: np.ndarray, max_layers: int) -> np.ndarray:
    """Start entry of every packet's chain in a DENSE layer array (PCPPX_LAYOUT_DENSE): the chains of the packets
    before it, whole batch."""
    cnt = np.minimum(n_layers.astype(np.int64), max_layers)
    return np.cumsum(cnt) - cnt


def unpack_dense(n_layers: np.ndarray, dense: np.ndarray, max_layers: int) -> np.ndarray:
    """DENSE layer entries -> the FIXED [n, max_layers] array (entries past a chain zero)."""
    n = len(n_layers)
    out = np.zeros((n, max_layers), dtype=LAYER_DTYPE)
    if n == 0 or max_layers == 0:
        return out
    cnt = np.minimum(n_layers.astype(np.int64), max_layers)
    start = dense_positions(n_layers, max_layers)
    flat = dense.reshape(-1)
    for k in range(max_layers):
        m = cnt > k
        out[m, k] = flat[start[m] + k]
    return out


def chain_proto_mask(fixed: np.ndarray, n_layers: np.ndarray) -> np.ndarray:
    """pcppx_chain_proto_mask over FIXED rows: Packet::isPacketOfType's mask from the recorded chain."""
    n, ml = fixed.shape
    k = np.arange(ml)[None, :] < np.minimum(n_layers.astype(np.int64), ml)[:, None]
    bits = np.where(k & (fixed["proto"] < 64), np.left_shift(np.uint64(1), fixed["proto"].astype(np.uint64)),
                    np.uint64(0))
    return np.bitwise_or.reduce(bits, axis=1) if ml else np.zeros(n, np.uint64)


def _declare(lib: C.CDLL) -> C.CDLL:
    P = C.c_void_p
    lib.pcppx_abi_version.restype = C.c_int
    lib.pcppx_strerror.restype = C.c_char_p
    lib.pcppx_strerror.argtypes = [C.c_int]
    lib.pcppx_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.pcppx_runtime_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    lib.pcppx_runtime_info.restype = C.c_int
    lib.pcppx_open.argtypes = [C.c_int, C.POINTER(P)]
    lib.pcppx_close.argtypes = [P]
    lib.pcppx_close.restype = None
    lib.pcppx_sync.argtypes = [P]
    lib.pcppx_ctx_stream.argtypes = [P]
    lib.pcppx_ctx_stream.restype = P
    lib.pcppx_default_opts.argtypes = [C.POINTER(Opts)]
    lib.pcppx_default_opts.restype = None
    lib.pcppx_parse_batch_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Opts), C.POINTER(Records), P]
    lib.pcppx_parse_batch_host.argtypes = [P, C.POINTER(Batch), C.POINTER(Opts), C.POINTER(Records)]
    lib.pcppx_flow_count_device.argtypes = [P, P, P, C.c_uint32, P, P, P, C.c_uint32, P, P]
    lib.pcppx_flow_count_keys_device.argtypes = [P, P, P, C.c_uint32, P, P, P, C.c_uint32, P, P]
    lib.pcppx_flow_count_keys_device.restype = C.c_int
    lib.pcppx_filter_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(MatchSpec),
                                        C.c_uint64, P, P, C.c_uint32, P, P, P]
    lib.pcppx_filter_device.restype = C.c_int
    lib.pcppx_reasm_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P, P]
    lib.pcppx_reasm_device.restype = C.c_int
    lib.pcppx_parse_batch_device_reasm.argtypes = [P, C.POINTER(Batch), C.POINTER(Opts), C.POINTER(Records), P, P]
    lib.pcppx_parse_batch_device_reasm.restype = C.c_int
    lib.pcppx_filter_reset.argtypes = [P, C.c_uint32]
    lib.pcppx_filter_reset.restype = C.c_int
    lib.pcppx_filter_batch_host.argtypes = [P, C.POINTER(Batch), C.POINTER(MatchSpec), P, C.POINTER(PacketStats)]
    lib.pcppx_filter_batch_host.restype = C.c_int
    lib.pcppx_pcap_open.argtypes = [C.c_char_p, C.POINTER(P)]
    lib.pcppx_pcap_open.restype = C.c_int
    lib.pcppx_pcap_linktype.argtypes = [P]
    lib.pcppx_pcap_linktype.restype = C.c_uint32
    lib.pcppx_pcap_read_batch.argtypes = [P, P, C.c_uint64, P, P, P, C.c_uint32, C.POINTER(C.c_uint32),
                                          C.POINTER(C.c_uint64)]
    lib.pcppx_pcap_read_batch.restype = C.c_int
    lib.pcppx_pcap_read_batch_ex.argtypes = [P, P, C.c_uint64, P, P, P, P, C.c_uint32, C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64)]
    lib.pcppx_pcap_read_batch_ex.restype = C.c_int
    lib.pcppx_pcap_map_batch.argtypes = [P, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), P, P, P, P, C.c_uint32,
                                         C.POINTER(C.c_uint32)]
    lib.pcppx_pcap_map_batch.restype = C.c_int
    lib.pcppx_pcap_close.argtypes = [P]
    lib.pcppx_pcap_close.restype = None
    lib.pcppx_host_alloc.argtypes = [C.c_size_t]
    lib.pcppx_host_alloc.restype = P
    lib.pcppx_host_free.argtypes = [P]
    lib.pcppx_host_free.restype = None
    lib.pcppx_unpack_layers.argtypes = [P, P, C.c_uint64, C.c_uint32, P]
    lib.pcppx_unpack_layers.restype = C.c_int
    lib.pcppx_window_choice.argtypes = [P, C.c_int, C.POINTER(C.c_int)]
    lib.pcppx_window_choice.restype = C.c_int
    lib.pcppx_unpack_layers_brief.argtypes = [P, P, C.c_uint64, C.c_uint32, P]
    lib.pcppx_unpack_layers_brief.restype = C.c_int
    lib.pcppx_select_device.argtypes = [P, C.POINTER(Batch), C.POINTER(SelectSpec), C.POINTER(Selection), P]
    lib.pcppx_select_device.restype = C.c_int
    lib.pcppx_select_reference.argtypes = [C.POINTER(Batch), C.POINTER(SelectSpec), C.POINTER(Selection)]
    lib.pcppx_select_reference.restype = C.c_int
    lib.pcppx_steer_device.argtypes = [P, C.POINTER(Batch), C.POINTER(SteerSpec), C.POINTER(Steering), P]
    lib.pcppx_steer_device.restype = C.c_int
    lib.pcppx_steer_reference.argtypes = [C.POINTER(Batch), C.POINTER(SteerSpec), C.POINTER(Steering)]
    lib.pcppx_steer_reference.restype = C.c_int
    lib.pcppx_defrag_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P, C.POINTER(DefragSpec),
                                        C.POINTER(Defragged), P]
    lib.pcppx_defrag_device.restype = C.c_int
    lib.pcppx_defrag_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P, C.POINTER(DefragSpec),
                                           C.POINTER(Defragged)]
    lib.pcppx_defrag_reference.restype = C.c_int
    lib.pcppx_defrag6_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P,
                                         C.POINTER(Defrag6Spec), C.POINTER(Defragged), P]
    lib.pcppx_defrag6_device.restype = C.c_int
    lib.pcppx_defrag6_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P,
                                            C.POINTER(Defrag6Spec), C.POINTER(Defragged)]
    lib.pcppx_defrag6_reference.restype = C.c_int
    lib.pcppx_tcpstream_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P,
                                           C.POINTER(TcpStreamSpec), C.POINTER(TcpStreams), P]
    lib.pcppx_tcpstream_device.restype = C.c_int
    lib.pcppx_tcpstream_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, P,
                                              C.POINTER(TcpStreamSpec), C.POINTER(TcpStreams)]
    lib.pcppx_tcpstream_reference.restype = C.c_int
    lib.pcppx_frag_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(FragSpec),
                                      C.POINTER(Fragmented), P]
    lib.pcppx_frag_device.restype = C.c_int
    lib.pcppx_frag_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(FragSpec),
                                         C.POINTER(Fragmented)]
    lib.pcppx_frag_reference.restype = C.c_int
    lib.pcppx_frag6_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(Frag6Spec),
                                       C.POINTER(Fragmented), P]
    lib.pcppx_frag6_device.restype = C.c_int
    lib.pcppx_frag6_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(Frag6Spec),
                                          C.POINTER(Fragmented)]
    lib.pcppx_frag6_reference.restype = C.c_int
    lib.pcppx_tlsfp_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(TlsfpSpec),
                                       C.POINTER(Tlsfps), P]
    lib.pcppx_tlsfp_device.restype = C.c_int
    lib.pcppx_tlsfp_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(TlsfpSpec),
                                          C.POINTER(Tlsfps)]
    lib.pcppx_tlsfp_reference.restype = C.c_int
    lib.pcppx_dns_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(DnsSpec),
                                     C.POINTER(DnsOut), P]
    lib.pcppx_dns_device.restype = C.c_int
    lib.pcppx_dns_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(DnsSpec),
                                        C.POINTER(DnsOut)]
    lib.pcppx_dns_reference.restype = C.c_int
    lib.pcppx_http_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(HttpSpec),
                                      C.POINTER(HttpOut), P]
    lib.pcppx_http_device.restype = C.c_int
    lib.pcppx_http_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(HttpSpec),
                                         C.POINTER(HttpOut)]
    lib.pcppx_http_reference.restype = C.c_int
    lib.pcppx_ssl_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(SslSpec),
                                     C.POINTER(SslOut), P]
    lib.pcppx_ssl_device.restype = C.c_int
    lib.pcppx_ssl_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(SslSpec),
                                        C.POINTER(SslOut)]
    lib.pcppx_ssl_reference.restype = C.c_int
    lib.pcppx_sip_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(HttpSpec),
                                     C.POINTER(SipOut), P]
    lib.pcppx_sip_device.restype = C.c_int
    lib.pcppx_sip_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(HttpSpec),
                                        C.POINTER(SipOut)]
    lib.pcppx_sip_reference.restype = C.c_int
    lib.pcppx_dhcp_device.argtypes = [P, C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(DhcpSpec),
                                      C.POINTER(DhcpOut), P]
    lib.pcppx_dhcp_device.restype = C.c_int
    lib.pcppx_dhcp_reference.argtypes = [C.POINTER(Batch), C.POINTER(Records), C.c_uint8, C.POINTER(DhcpSpec),
                                         C.POINTER(DhcpOut)]
    lib.pcppx_dhcp_reference.restype = C.c_int
    lib.pcppx_bpf_validate.argtypes = [P, C.c_uint32]
    lib.pcppx_bpf_validate.restype = C.c_int
    lib.pcppx_bpf_load.argtypes = [P, P, C.c_uint32, C.POINTER(P)]
    lib.pcppx_bpf_load.restype = C.c_int
    lib.pcppx_bpf_free.argtypes = [P]
    lib.pcppx_bpf_free.restype = None
    lib.pcppx_bpf_device.argtypes = [P, P, C.POINTER(Batch), P, C.POINTER(BpfVerdicts), P]
    lib.pcppx_bpf_device.restype = C.c_int
    lib.pcppx_bpf_reference.argtypes = [P, C.c_uint32, C.POINTER(Batch), P, C.POINTER(BpfVerdicts)]
    lib.pcppx_bpf_reference.restype = C.c_int
    for name in ("pcppx_device_count", "pcppx_open", "pcppx_sync", "pcppx_parse_batch_device",
                 "pcppx_parse_batch_host", "pcppx_flow_count_device"):
        getattr(lib, name).restype = C.c_int
    return lib


_ENGINE: C.CDLL | None = None

# every symbol include/pcppx.h declares
EXPORTED_SYMBOLS = (
    "pcppx_abi_version", "pcppx_strerror", "pcppx_device_count", "pcppx_runtime_info", "pcppx_open", "pcppx_close",
    "pcppx_sync", "pcppx_ctx_stream", "pcppx_default_opts", "pcppx_parse_batch_device", "pcppx_parse_batch_host",
    "pcppx_flow_count_device", "pcppx_flow_count_keys_device", "pcppx_filter_device", "pcppx_filter_reset", "pcppx_filter_batch_host", "pcppx_reasm_device", "pcppx_parse_batch_device_reasm", "pcppx_pcap_open", "pcppx_pcap_linktype",
    "pcppx_pcap_read_batch", "pcppx_pcap_read_batch_ex", "pcppx_pcap_map_batch", "pcppx_pcap_close", "pcppx_host_alloc", "pcppx_host_free",
    "pcppx_unpack_layers", "pcppx_unpack_layers_brief", "pcppx_window_choice",
    "pcppx_select_device", "pcppx_select_reference", "pcppx_steer_device", "pcppx_steer_reference",
    "pcppx_defrag_device", "pcppx_defrag_reference", "pcppx_defrag6_device", "pcppx_defrag6_reference",
    "pcppx_frag_device", "pcppx_frag_reference", "pcppx_frag6_device", "pcppx_frag6_reference",
    "pcppx_tcpstream_device", "pcppx_tcpstream_reference", "pcppx_tlsfp_device", "pcppx_tlsfp_reference",
    "pcppx_dns_device", "pcppx_dns_reference",
    "pcppx_http_device", "pcppx_http_reference",
    "pcppx_ssl_device", "pcppx_ssl_reference",
    "pcppx_sip_device", "pcppx_sip_reference",
    "pcppx_dhcp_device", "pcppx_dhcp_reference",
    "pcppx_bpf_validate", "pcppx_bpf_load", "pcppx_bpf_free", "pcppx_bpf_device", "pcppx_bpf_reference",
)


def load_engine() -> C.CDLL:
    """Load the HIP engine (pcapplusplus_amd/libpcppx.so). Raises if it has not been built."""
    global _ENGINE
    if _ENGINE is None:
        if not ENGINE_SO.exists():
            raise RuntimeError(
                f"HIP engine library {ENGINE_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                " (or `make -C pcapplusplus_amd/csrc`). There is no CPU fallback.")
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7. Importing torch first makes
        # the engine bind to that same runtime (matched by SONAME), so torch tensors/streams and the
        # engine's kernels share one device context.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = _declare(C.CDLL(str(ENGINE_SO)))
        if lib.pcppx_abi_version() != ABI_VERSION:
            raise RuntimeError("libpcppx.so ABI version mismatch")
        _ENGINE = lib
    return _ENGINE


def runtime_info(device: int = 0) -> str:
    buf = C.create_string_buffer(256)
    load_engine().pcppx_runtime_info(device, buf, 256)
    return buf.value.decode()


def check(rc: int, what: str = "pcppx") -> None:
    if rc != OK:
        msg = load_engine().pcppx_strerror(rc).decode() if _ENGINE is not None else str(rc)
        raise RuntimeError(f"{what} failed: {msg} ({rc})")


def ptr(a) -> int:
    """Data pointer of a numpy array or torch tensor."""
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


__all__ = [n for n in dir() if not n.startswith("_")]
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
