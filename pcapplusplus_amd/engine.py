"""Engine handle: one pcppx context (one GPU, one host thread) over the C ABI of include/pcppx.h.

Host batches (numpy) go through pcppx_parse_batch_host (pinned, double-buffered H2D -> kernel -> D2H);
device batches (torch tensors resident in HBM) through pcppx_parse_batch_device on a HIP stream.
There is no CPU fallback: a missing libpcppx.so or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .pcap import PacketBatch


def _opt(t):
    """An optional tensor's address."""
    return abi.ptr(t) if t is not None else None


def _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len):
    """The (abi.Batch, abi.Records) of a device batch and its parse's records (summary or brief; FIXED layers) as the
    operators over parsed packets take them; data_len None: all of data."""
    b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens),
                  int(data.numel()) if data_len is None else data_len, n, linktype, 0)
    rec = abi.Records(_opt(summary), abi.ptr(layers))
    rec.brief = _opt(brief)
    return b, rec


class Engine:
    def __init__(self, device: int = 0):
        self.lib = abi.load_engine()
        self.ctx = C.c_void_p()
        abi.check(self.lib.pcppx_open(device, C.byref(self.ctx)), "pcppx_open")
        self.device = device

    def close(self) -> None:
        if self.ctx:
            self.lib.pcppx_close(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-resident batches ----
    def parse_host(self, batch: PacketBatch, opts: abi.Opts | None = None, out=None):
        """Parse a host batch; returns (summary[n], layers[n, max_layers]) numpy record arrays. out: caller-owned
        (summary, layers) arrays to fill (e.g. pinned_records(): the records then come back by DMA straight
        into them), else fresh zeroed arrays."""
        opts = opts or abi.make_opts()
        if out is None:
            summary = np.zeros(batch.n, dtype=abi.SUMMARY_DTYPE)
            layers = np.zeros(max(batch.n * opts.max_layers, 1), dtype=abi.LAYER_DTYPE)
        else:
            summary, layers = out
            if summary.shape[0] < batch.n or layers.size < batch.n * opts.max_layers:
                raise ValueError("output arrays too small for the batch")
        rec = abi.Records(summary.ctypes.data, layers.ctypes.data if opts.max_layers else None)
        b = batch.c_batch()
        abi.check(self.lib.pcppx_parse_batch_host(self.ctx, C.byref(b), C.byref(opts), C.byref(rec)),
                  "pcppx_parse_batch_host")
        return summary, layers[: batch.n * opts.max_layers].reshape(batch.n, opts.max_layers)

    def parse_host_ex(self, batch: PacketBatch, opts: abi.Opts, want_summary: bool = True, want_brief: bool = False,
                      pinned: bool = False):
        """Host parse with the ABI-7 outputs: the summary and / or the 16-B brief, and the layer entries in opts.layout
        (LAYOUT_FIXED: [n, max_layers]; LAYOUT_DENSE: the chains back to back, pcppx_records.layers_written of them).
        Returns (summary | None, brief | None, layers, layers_written). pinned: page-locked output arrays (records
        DMA'd straight into them)."""
        n, ml = batch.n, opts.max_layers
        keep = []

        def arr(count, dt):
            if not pinned:
                return np.zeros(count, dtype=dt)
            buf = PinnedBuffer(max(count, 1) * dt.itemsize)
            keep.append(buf)
            return buf.array.view(dt)[:count]

        summary = arr(n, abi.SUMMARY_DTYPE) if want_summary else None
        brief = arr(n, abi.BRIEF_DTYPE) if want_brief else None
        layers = arr(max(n * ml, 1), abi.LAYER_DTYPE)
        rec = abi.Records(summary.ctypes.data if summary is not None else None, layers.ctypes.data if ml else None)
        rec.brief = brief.ctypes.data if brief is not None else None
        b = batch.c_batch()
        abi.check(self.lib.pcppx_parse_batch_host(self.ctx, C.byref(b), C.byref(opts), C.byref(rec)),
                  "pcppx_parse_batch_host")
        w = int(rec.layers_written)
        out = (None if summary is None else summary.copy() if pinned else summary,
               None if brief is None else brief.copy() if pinned else brief,
               layers[:w].copy() if pinned else layers[:w], w)
        for k in keep:
            k.free()
        return out

    def window_choice(self, want_checksums: bool) -> int:
        """pcppx_window_choice: the window a WINDOW_DEFAULT launch would run with now (abi.WINDOW_*)."""
        w = C.c_int(0)
        abi.check(self.lib.pcppx_window_choice(self.ctx, 1 if want_checksums else 0, C.byref(w)), "pcppx_window_choice")
        return w.value

    # ---- device-resident batches (torch tensors on this GPU) ----
    def parse_device(self, data, offsets, caplens, n: int, linktype: int, opts: abi.Opts, summary, layers=None,
                     stream: int | None = None, flow_keys=None, tuples=None, proto_stats=None, brief=None) -> None:
        """Queue a parse of device tensors on `stream` (a hipStream_t handle, e.g.
        torch.cuda.current_stream().cuda_stream). summary: uint8 tensor of n*32 bytes (or None with no layers when
        tuples / flow_keys / proto_stats is given); layers: n*max_layers*8; flow_keys: n int32 (hash5); tuples: n*48
        bytes (5-tuple extracts); proto_stats: 16 x int64, accumulated (collectStats)."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens), int(data.numel()), n, linktype, 0)
        rec = abi.Records(_opt(summary), abi.ptr(layers) if (layers is not None and opts.max_layers) else None,
                          _opt(flow_keys), _opt(tuples), _opt(proto_stats))
        rec.brief = _opt(brief)
        abi.check(self.lib.pcppx_parse_batch_device(self.ctx, C.byref(b), C.byref(opts), C.byref(rec),
                                                    C.c_void_p(stream or 0)), "pcppx_parse_batch_device")

    def flow_count_device(self, summary, caplens, n: int, keys, packets, bytes_, capacity: int, stats,
                          stream: int | None = None) -> None:
        abi.check(self.lib.pcppx_flow_count_device(self.ctx, abi.ptr(summary), abi.ptr(caplens), n, abi.ptr(keys),
                                                   abi.ptr(packets), abi.ptr(bytes_), capacity, abi.ptr(stats),
                                                   C.c_void_p(stream or 0)), "pcppx_flow_count_device")

    def flow_count_keys_device(self, flow_keys, caplens, n: int, keys, packets, bytes_, capacity: int, stats,
                               stream: int | None = None) -> None:
        """pcppx_flow_count_keys_device: the flow table over the dense hash5 column a parse wrote (flow_keys)."""
        abi.check(self.lib.pcppx_flow_count_keys_device(self.ctx, abi.ptr(flow_keys), abi.ptr(caplens), n, abi.ptr(keys),
                                                        abi.ptr(packets), abi.ptr(bytes_), capacity, abi.ptr(stats),
                                                        C.c_void_p(stream or 0)), "pcppx_flow_count_keys_device")

    def filter_device(self, data, offsets, caplens, n: int, linktype: int, summary, layers, max_layers: int,
                      spec: abi.MatchSpec, seq_base: int, flow_keys, flow_first, capacity: int, matched, stats,
                      stream: int | None = None) -> None:
        """FilterTraffic's worker over a parsed device batch (pcppx_filter_device). flow_keys/flow_first:
        zero-initialised u64 tensors of `capacity` (power of two) slots kept across batches; matched: u8[n];
        stats: 14 x u64 (abi.STATS_FIELDS order), accumulated."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens), int(data.numel()), n, linktype, 0)
        rec = abi.Records(abi.ptr(summary), abi.ptr(layers))
        abi.check(self.lib.pcppx_filter_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                               seq_base, abi.ptr(flow_keys), abi.ptr(flow_first), capacity,
                                               abi.ptr(matched), abi.ptr(stats), C.c_void_p(stream or 0)),
                  "pcppx_filter_device")

    def reasm_device(self, data, offsets, caplens, n: int, linktype: int, summary, layers, max_layers: int, info,
                     stream: int | None = None) -> None:
        """The reassembly front ends (pcppx_reasm_device) over a parsed device batch: info is a uint8 tensor of
        n * 16 bytes (abi.REASM_DTYPE records)."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens), int(data.numel()), n, linktype, 0)
        rec = abi.Records(abi.ptr(summary), abi.ptr(layers))
        abi.check(self.lib.pcppx_reasm_device(self.ctx, C.byref(b), C.byref(rec), max_layers, abi.ptr(info),
                                              C.c_void_p(stream or 0)), "pcppx_reasm_device")

    def parse_reasm_device(self, data, offsets, caplens, n: int, linktype: int, opts: abi.Opts, summary, layers,
                           info, stream: int | None = None) -> None:
        """Parse + reassembly front ends in one kernel pass (pcppx_parse_batch_device_reasm)."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens), int(data.numel()), n, linktype, 0)
        rec = abi.Records(abi.ptr(summary), abi.ptr(layers))
        abi.check(self.lib.pcppx_parse_batch_device_reasm(self.ctx, C.byref(b), C.byref(opts), C.byref(rec),
                                                          abi.ptr(info), C.c_void_p(stream or 0)),
                  "pcppx_parse_batch_device_reasm")

    def select_device(self, data, offsets, caplens, n: int, linktype: int, spec: abi.SelectSpec, out_offsets,
                      out_caplens, totals, max_packets: int, out_data=None, data_cap: int = 0, out_index=None,
                      stream: int | None = None, data_len: int | None = None) -> None:
        """Queue pcppx_select_device over device tensors: the packets spec selects (abi.make_select_spec: a keep mask,
        or the flags of a parse's summary / brief) are gathered in source order into out_data (u8, data_cap bytes; None
        = index-only) with out_offsets (i64) / out_caplens (i32) / out_index (i32, optional) of max_packets entries;
        totals: 8 x i64 (abi.SEL_*), overwritten. Returns without waiting."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens),
                      int(data.numel()) if data_len is None else data_len, n, linktype, 0)
        sel = abi.Selection(_opt(out_data), data_cap, abi.ptr(out_offsets), abi.ptr(out_caplens), _opt(out_index),
                            max_packets, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_select_device(self.ctx, C.byref(b), C.byref(spec), C.byref(sel),
                                               C.c_void_p(stream or 0)), "pcppx_select_device")

    def steer_device(self, data, offsets, caplens, n: int, linktype: int, spec: abi.SteerSpec, out_offsets,
                     out_caplens, bucket_first, bucket_pos, totals, max_packets: int, out_data=None, data_cap: int = 0,
                     out_index=None, stream: int | None = None, data_len: int | None = None) -> None:
        """Queue pcppx_steer_device over device tensors: the packets go, bucket by bucket (abi.make_steer_spec: a
        bucket column, or a 32-bit key % n_buckets) and in source order inside a bucket, into out_data (u8, data_cap
        bytes; None = index-only) with out_offsets (i64) / out_caplens (i32) / out_index (i32, optional) of max_packets
        entries; bucket_first (i32) / bucket_pos (i64): n_buckets + 1 entries; totals: 8 x i64 (abi.STEER_*),
        overwritten. All or nothing: on overflow only totals / bucket_first / bucket_pos are written. Returns without
        waiting."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens),
                      int(data.numel()) if data_len is None else data_len, n, linktype, 0)
        out = abi.Steering(_opt(out_data), data_cap, abi.ptr(out_offsets), abi.ptr(out_caplens), _opt(out_index),
                           abi.ptr(bucket_first), abi.ptr(bucket_pos), max_packets, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_steer_device(self.ctx, C.byref(b), C.byref(spec), C.byref(out),
                                              C.c_void_p(stream or 0)), "pcppx_steer_device")

    def defrag_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, info,
                      spec: abi.DefragSpec, out_offsets, out_caplens, totals, max_packets: int, out_data=None,
                      data_cap: int = 0, out_index=None, out_first=None, out_frags=None, disposition=None,
                      stream: int | None = None, data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_defrag_device over device tensors: the IPv4 fragment groups that are complete and well formed
        inside the batch are reassembled; with spec.passthrough every other packet is copied in place. summary (n * 32
        bytes) or brief (n * 16 bytes): the parse's records, one of them; layers: FIXED, n * max_layers
        * 8 bytes; info: n * 16 bytes (abi.REASM_DTYPE). out_data (u8, data_cap bytes; None = index-only), out_offsets
        (i64) / out_caplens (i32) / out_index / out_first (i32) / out_frags (u8) of max_packets entries, disposition
        (u8[n]), each of the last four optional; totals: 8 x i64 (abi.DEFRAG_*), overwritten. All or nothing: on
        overflow only the totals are written. Returns without waiting."""
        self._defrag("pcppx_defrag_device", data, offsets, caplens, n, linktype, layers, max_layers, info, spec,
                     out_offsets, out_caplens, totals, max_packets, out_data, data_cap, out_index, out_first, out_frags,
                     disposition, stream, data_len, summary, brief)

    def defrag6_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, info,
                       spec: abi.Defrag6Spec, out_offsets, out_caplens, totals, max_packets: int, out_data=None,
                       data_cap: int = 0, out_index=None, out_first=None, out_frags=None, disposition=None,
                       stream: int | None = None, data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_defrag6_device over device tensors: defrag_device for the families spec.families names (the
        IPv6 fragment groups are reassembled too). The arguments are defrag_device's."""
        self._defrag("pcppx_defrag6_device", data, offsets, caplens, n, linktype, layers, max_layers, info, spec,
                     out_offsets, out_caplens, totals, max_packets, out_data, data_cap, out_index, out_first, out_frags,
                     disposition, stream, data_len, summary, brief)

    def _defrag(self, call: str, data, offsets, caplens, n, linktype, layers, max_layers, info, spec, out_offsets,
                out_caplens, totals, max_packets, out_data, data_cap, out_index, out_first, out_frags, disposition,
                stream, data_len, summary, brief) -> None:
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.Defragged(_opt(out_data), data_cap, abi.ptr(out_offsets), abi.ptr(out_caplens), _opt(out_index),
                            _opt(out_first), _opt(out_frags), _opt(disposition), max_packets, 0, abi.ptr(totals))
        abi.check(getattr(self.lib, call)(self.ctx, C.byref(b), C.byref(rec), max_layers, abi.ptr(info),
                                          C.byref(spec), C.byref(out), C.c_void_p(stream or 0)), call)

    def tcpstream_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, info,
                         spec: abi.TcpStreamSpec, streams, totals, max_streams: int, out_data=None, data_cap: int = 0,
                         disposition=None, seg_stream=None, seg_pos=None, stream: int | None = None,
                         data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_tcpstream_device over device tensors: the TCP connection sides that are clean inside the batch
        are reassembled into contiguous stream bytes. summary (n * 32 bytes) or brief (n * 16 bytes): the parse's
        records, one of them; layers: FIXED, n * max_layers * 8 bytes; info: n * 16 bytes (abi.REASM_DTYPE). out_data
        (u8, data_cap bytes; None = index-only), streams (max_streams * 32 bytes, abi.TCPSTREAM_DTYPE), disposition
        (u8[n]) / seg_stream / seg_pos (i32[n]) optional; totals: 8 x i64 (abi.TCPS_*), overwritten. All or nothing:
        on overflow only the totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.TcpStreams(_opt(out_data), data_cap, abi.ptr(streams), _opt(disposition), _opt(seg_stream),
                             _opt(seg_pos), max_streams, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_tcpstream_device(self.ctx, C.byref(b), C.byref(rec), max_layers, abi.ptr(info),
                                                  C.byref(spec), C.byref(out), C.c_void_p(stream or 0)),
                  "pcppx_tcpstream_device")

    def frag_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, spec: abi.FragSpec,
                    out_offsets, out_caplens, totals, max_packets: int, out_data=None, data_cap: int = 0,
                    out_index=None, out_frag_no=None, counts=None, disposition=None, stream: int | None = None,
                    data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_frag_device over device tensors: the IPv4 packets spec chooses (abi.make_frag_spec) whose IP
        payload exceeds the fragment size are split into fragments in place; with spec.copy_rest every other packet is
        copied. summary (n * 32 bytes) or brief (n * 16 bytes): the parse's records, one of them; layers: FIXED,
        n * max_layers * 8 bytes. out_data (u8, data_cap bytes; None = index-only), out_offsets (i64) / out_caplens
        (i32) / out_index (i32) / out_frag_no (i16) of max_packets entries, counts (i16[n]), disposition (u8[n]), each
        of the last four optional; totals: 8 x i64 (abi.FRAG_*), overwritten. All or nothing: on overflow only the
        totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.Fragmented(_opt(out_data), data_cap, abi.ptr(out_offsets), abi.ptr(out_caplens), _opt(out_index),
                             _opt(out_frag_no), _opt(counts), _opt(disposition), max_packets, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_frag_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                             C.byref(out), C.c_void_p(stream or 0)), "pcppx_frag_device")

    def frag6_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int,
                     spec: abi.Frag6Spec, out_offsets, out_caplens, totals, max_packets: int, out_data=None,
                     data_cap: int = 0, out_index=None, out_frag_no=None, counts=None, disposition=None,
                     stream: int | None = None, data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_frag6_device over device tensors: frag_device for the families spec.families names (the IPv6
        packets are split too, with the fragment ids of spec.ids / spec.id_base). The arguments are frag_device's."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.Fragmented(_opt(out_data), data_cap, abi.ptr(out_offsets), abi.ptr(out_caplens), _opt(out_index),
                             _opt(out_frag_no), _opt(counts), _opt(disposition), max_packets, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_frag6_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                              C.byref(out), C.c_void_p(stream or 0)), "pcppx_frag6_device")

    def tlsfp_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int,
                     spec: abi.TlsfpSpec, recs, totals, max_recs: int, text=None, text_cap: int = 0, disposition=None,
                     stream: int | None = None, data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_tlsfp_device over device tensors: one record (abi.TLSFP_REC_DTYPE, 40 bytes) per ClientHello /
        ServerHello packet spec asks for, with the MD5 of its JA3 / JA3S text. summary (n * 32 bytes) or brief (n * 16
        bytes): the parse's records, one of them; layers: FIXED, n * max_layers * 8 bytes. recs: max_recs * 40 bytes;
        text (u8, text_cap bytes; None = MD5 only); disposition (u8[n], optional); totals: 8 x i64 (abi.TLSFP_*),
        overwritten. All or nothing: on overflow only the totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.Tlsfps(abi.ptr(recs), _opt(text), text_cap, _opt(disposition), max_recs, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_tlsfp_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                              C.byref(out), C.c_void_p(stream or 0)), "pcppx_tlsfp_device")

    def dns_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, spec: abi.DnsSpec,
                   msgs, rrs, totals, max_msgs: int, max_rrs: int, names=None, names_cap: int = 0, disposition=None,
                   stream: int | None = None, data_len: int | None = None, summary=None, brief=None) -> None:
        """Queue pcppx_dns_device over device tensors: one message (abi.DNS_MSG_DTYPE, 40 bytes) per DNS packet and one
        record (abi.DNS_RR_DTYPE, 32 bytes) per linked resource of the sections spec asks for, with its decoded name.
        summary (n * 32 bytes) or brief (n * 16 bytes): the parse's records, one of them; layers: FIXED,
        n * max_layers * 8 bytes. msgs: max_msgs * 40 bytes; rrs: max_rrs * 32 bytes; names (u8, names_cap bytes; None =
        no text); disposition (u8[n], optional); totals: 8 x i64 (abi.DNS_*), overwritten. All or nothing: on overflow
        only the totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.DnsOut(abi.ptr(msgs), abi.ptr(rrs), _opt(names), names_cap, _opt(disposition), max_msgs, max_rrs,
                         abi.ptr(totals))
        abi.check(self.lib.pcppx_dns_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                            C.byref(out), C.c_void_p(stream or 0)), "pcppx_dns_device")

    def http_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, spec: abi.HttpSpec,
                    msgs, fields, totals, max_msgs: int, max_fields: int, text=None, text_cap: int = 0,
                    disposition=None, stream: int | None = None, data_len: int | None = None, summary=None,
                    brief=None) -> None:
        """Queue pcppx_http_device over device tensors: one message (abi.HTTP_MSG_DTYPE, 48 bytes) per HTTP packet and
        one record (abi.HTTP_FIELD_DTYPE, 24 bytes) per header field spec asks for, with the bytes spec asks for.
        summary (n * 32 bytes) or brief (n * 16 bytes): the parse's records, one of them; layers: FIXED,
        n * max_layers * 8 bytes. msgs: max_msgs * 48 bytes; fields: max_fields * 24 bytes; text (u8, text_cap bytes;
        None = no text); disposition (u8[n], optional); totals: 12 x i64 (abi.HTTP_*), overwritten. All or nothing: on
        overflow only the totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.HttpOut(abi.ptr(msgs), abi.ptr(fields), _opt(text), text_cap, _opt(disposition), max_msgs, max_fields,
                          abi.ptr(totals))
        abi.check(self.lib.pcppx_http_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                             C.byref(out), C.c_void_p(stream or 0)), "pcppx_http_device")

    def ssl_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, spec: abi.SslSpec,
                   msgs, hellos, totals, max_msgs: int, max_hellos: int, names=None, names_cap: int = 0,
                   disposition=None, stream: int | None = None, data_len: int | None = None, summary=None,
                   brief=None) -> None:
        """Queue pcppx_ssl_device over device tensors: one message (abi.SSL_MSG_DTYPE, 32 bytes) per SSL packet and one
        record (abi.SSL_HELLO_DTYPE, 32 bytes) per ClientHello / ServerHello spec asks for, with the SNI host names.
        summary (n * 32 bytes) or brief (n * 16 bytes): the parse's records, one of them; layers: FIXED,
        n * max_layers * 8 bytes. msgs: max_msgs * 32 bytes; hellos: max_hellos * 32 bytes; names (u8, names_cap bytes;
        None = positions only); disposition (u8[n], optional); totals: 12 x i64 (abi.SSL_*), overwritten. All or
        nothing: on overflow only the totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.SslOut(abi.ptr(msgs), abi.ptr(hellos), _opt(names), names_cap, _opt(disposition), max_msgs, max_hellos,
                         abi.ptr(totals))
        abi.check(self.lib.pcppx_ssl_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                            C.byref(out), C.c_void_p(stream or 0)), "pcppx_ssl_device")

    def sip_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, spec: abi.SipSpec,
                   msgs, fields, sdps, totals, max_msgs: int, max_fields: int, max_sdps: int, text=None,
                   text_cap: int = 0, disposition=None, stream: int | None = None, data_len: int | None = None,
                   summary=None, brief=None) -> None:
        """Queue pcppx_sip_device over device tensors: one message (abi.SIP_MSG_DTYPE, 48 bytes) per SIP packet, one
        record (abi.SIP_FIELD_DTYPE, 24 bytes) per header field spec asks for with the bytes spec asks for, and one
        record (abi.SIP_SDP_DTYPE, 32 bytes) per SDP body. summary (n * 32 bytes) or brief (n * 16 bytes): the parse's
        records, one of them; layers: FIXED, n * max_layers * 8 bytes. msgs: max_msgs * 48 bytes; fields: max_fields *
        24 bytes; sdps: max_sdps * 32 bytes; text (u8, text_cap bytes; None = no text); disposition (u8[n], optional);
        totals: 12 x i64 (abi.SIP_*), overwritten. All or nothing: on overflow only the totals are written. Returns
        without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.SipOut(abi.ptr(msgs), abi.ptr(fields), abi.ptr(sdps), _opt(text), text_cap, _opt(disposition),
                         max_msgs, max_fields, max_sdps, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_sip_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                            C.byref(out), C.c_void_p(stream or 0)), "pcppx_sip_device")

    def dhcp_device(self, data, offsets, caplens, n: int, linktype: int, layers, max_layers: int, spec: abi.DhcpSpec,
                    msgs, options, totals, max_msgs: int, max_options: int, values=None, values_cap: int = 0,
                    disposition=None, stream: int | None = None, data_len: int | None = None, summary=None,
                    brief=None) -> None:
        """Queue pcppx_dhcp_device over device tensors: one message (abi.DHCP_MSG_DTYPE, 80 bytes) per DHCP / DHCPv6
        packet and one record (abi.DHCP_OPTION_DTYPE, 16 bytes) per option spec asks for, with the value bytes spec
        asks for. summary (n * 32 bytes) or brief (n * 16 bytes): the parse's records, one of them; layers: FIXED,
        n * max_layers * 8 bytes. msgs: max_msgs * 80 bytes; options: max_options * 16 bytes; values (u8, values_cap
        bytes; None = positions only); disposition (u8[n], optional); totals: 10 x i64 (abi.DHCP_*), overwritten. All
        or nothing: on overflow only the totals are written. Returns without waiting."""
        b, rec = _source(data, offsets, caplens, n, linktype, layers, summary, brief, data_len)
        out = abi.DhcpOut(abi.ptr(msgs), abi.ptr(options), _opt(values), values_cap, _opt(disposition), max_msgs,
                          max_options, 0, abi.ptr(totals))
        abi.check(self.lib.pcppx_dhcp_device(self.ctx, C.byref(b), C.byref(rec), max_layers, C.byref(spec),
                                             C.byref(out), C.c_void_p(stream or 0)), "pcppx_dhcp_device")

    def bpf_load(self, programs) -> "BpfFilter":
        """pcppx_bpf_load: validate 1..16 classic BPF programs (abi.BPF_INSN_DTYPE arrays or (code, jt, jf, k) rows; see
        pcapplusplus_amd.bpf) and copy them to this context's GPU. Raises on a program the validator refuses."""
        progs, keep = abi.make_bpf_progs(programs)
        h = C.c_void_p()
        abi.check(self.lib.pcppx_bpf_load(self.ctx, progs, len(keep), C.byref(h)), "pcppx_bpf_load")
        return BpfFilter(self.lib, h, len(keep))

    def bpf_device(self, flt: "BpfFilter", data, offsets, caplens, n: int, linktype: int, totals, matched=None,
                   bucket=None, ret=None, frame_lens=None, stream: int | None = None,
                   data_len: int | None = None) -> None:
        """Queue pcppx_bpf_device over device tensors: flt's programs run over every packet; matched (u8) / bucket (u8:
        the first accepting program, 0xFF = none) / ret (i32: its return value) of n entries, each optional; totals:
        8 x i64 (abi.BPF_*), overwritten; frame_lens: i32 wire lengths (None: the caplens). Returns without waiting."""
        b = abi.Batch(abi.ptr(data), abi.ptr(offsets), abi.ptr(caplens),
                      int(data.numel()) if data_len is None else data_len, n, linktype, 0)
        out = abi.BpfVerdicts(_opt(matched), _opt(bucket), _opt(ret), abi.ptr(totals))
        abi.check(self.lib.pcppx_bpf_device(self.ctx, flt.handle, C.byref(b), _opt(frame_lens), C.byref(out),
                                            C.c_void_p(stream or 0)), "pcppx_bpf_device")

    def filter_reset(self, capacity: int = 0) -> None:
        abi.check(self.lib.pcppx_filter_reset(self.ctx, capacity), "pcppx_filter_reset")

    def filter_host(self, batch: PacketBatch, spec: abi.MatchSpec):
        """FilterTraffic's worker over a host batch (context-held flow table): (matched u8[n], stats dict
        accumulated since the last filter_reset)."""
        matched = np.zeros(max(batch.n, 1), dtype=np.uint8)
        st = abi.PacketStats()
        b = batch.c_batch()
        abi.check(self.lib.pcppx_filter_batch_host(self.ctx, C.byref(b), C.byref(spec), matched.ctypes.data,
                                                   C.byref(st)), "pcppx_filter_batch_host")
        return matched[: batch.n], st.as_dict()

    def sync(self) -> None:
        abi.check(self.lib.pcppx_sync(self.ctx), "pcppx_sync")


class BpfFilter:
    """Validated BPF programs resident on an engine's GPU (a pcppx_bpf handle, from Engine.bpf_load)."""

    def __init__(self, lib, handle, n_programs: int):
        self.lib, self.handle, self.n_programs = lib, handle, n_programs

    def free(self) -> None:
        """pcppx_bpf_free: waits for queued work that uses the programs."""
        if self.handle:
            self.lib.pcppx_bpf_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PcapReader:
    """Native capture ingest (pcppx_pcap_*): records of a pcap / pcapng capture copied straight into packed
    batches. Mirrors IFileReaderDevice (Pcap++/header/PcapFileDevice.h) open / getNextPackets / close; each
    batch carries one link type (RawPacket::getLinkLayerType), its timestamps and frame lengths."""

    def __init__(self, path: str, pinned: bool = False):
        self.lib = abi.load_engine()
        self.handle = C.c_void_p()
        abi.check(self.lib.pcppx_pcap_open(str(path).encode(), C.byref(self.handle)), f"pcppx_pcap_open({path})")
        self.linktype = int(self.lib.pcppx_pcap_linktype(self.handle))
        self.pinned = pinned

    def read_batch(self, max_packets: int = 1 << 20, data_cap: int = 256 << 20) -> PacketBatch:
        """Next batch of at most max_packets packets / data_cap bytes (n == 0 at end of file)."""
        data = np.empty(data_cap, dtype=np.uint8)
        offsets = np.empty(max_packets, dtype=np.uint64)
        caplens = np.empty(max_packets, dtype=np.uint32)
        frame_lens = np.empty(max_packets, dtype=np.uint32)
        ts = np.empty(max_packets, dtype=np.uint64)
        n, used = C.c_uint32(0), C.c_uint64(0)
        abi.check(self.lib.pcppx_pcap_read_batch_ex(self.handle, data.ctypes.data, data_cap, offsets.ctypes.data,
                                                    caplens.ctypes.data, frame_lens.ctypes.data, ts.ctypes.data,
                                                    max_packets, C.byref(n), C.byref(used)), "pcppx_pcap_read_batch_ex")
        k = n.value
        self.linktype = int(self.lib.pcppx_pcap_linktype(self.handle))
        return PacketBatch(data[: used.value].copy(), offsets[:k].copy(), caplens[:k].copy(), self.linktype,
                           timestamps_ns=ts[:k].copy(), frame_lens=frame_lens[:k].copy())

    def map_batch(self, max_packets: int = 1 << 20):
        """Zero-copy next batch (pcppx_pcap_map_batch): (map address, file size, offsets, caplens, frame_lens, ts);
        the bytes stay in the reader's memory map until close()."""
        offsets = np.empty(max_packets, dtype=np.uint64)
        caplens = np.empty(max_packets, dtype=np.uint32)
        frame_lens = np.empty(max_packets, dtype=np.uint32)
        ts = np.empty(max_packets, dtype=np.uint64)
        base, size, n = C.c_void_p(), C.c_uint64(0), C.c_uint32(0)
        abi.check(self.lib.pcppx_pcap_map_batch(self.handle, C.byref(base), C.byref(size), offsets.ctypes.data,
                                                caplens.ctypes.data, frame_lens.ctypes.data, ts.ctypes.data,
                                                max_packets, C.byref(n)), "pcppx_pcap_map_batch")
        k = n.value
        self.linktype = int(self.lib.pcppx_pcap_linktype(self.handle))
        return base.value, size.value, offsets[:k].copy(), caplens[:k].copy(), frame_lens[:k].copy(), ts[:k].copy()

    def close(self) -> None:
        if self.handle:
            self.lib.pcppx_pcap_close(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PinnedBuffer:
    """Page-locked host memory (pcppx_host_alloc) viewed as a numpy uint8 array: a host batch whose bytes
    sit here is copied to HBM by DMA straight from it (no staging copy), as a NIC ring's buffers would be."""

    def __init__(self, nbytes: int):
        self.lib = abi.load_engine()
        self.ptr = self.lib.pcppx_host_alloc(max(1, nbytes))
        if not self.ptr:
            raise MemoryError(f"pcppx_host_alloc({nbytes}) failed")
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(self.ptr))

    def free(self) -> None:
        if self.ptr:
            self.array = None
            self.lib.pcppx_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pinned_records(n: int, max_layers: int):
    """(summary[n], layers[n * max_layers]) record arrays in page-locked memory, plus the buffers to keep alive:
    pcppx_parse_batch_host then writes the records by DMA, with no host copy."""
    sb = PinnedBuffer(n * abi.SUMMARY_DTYPE.itemsize)
    lb = PinnedBuffer(max(1, n * max_layers) * abi.LAYER_DTYPE.itemsize)
    return (sb.array.view(abi.SUMMARY_DTYPE)[:n], lb.array.view(abi.LAYER_DTYPE)[: max(1, n * max_layers)]), (sb, lb)


def pinned_copy(batch: PacketBatch) -> tuple[PacketBatch, PinnedBuffer]:
    """The same batch with its bytes in page-locked memory (keep the buffer alive while the batch is used)."""
    buf = PinnedBuffer(batch.data.nbytes)
    buf.array[: batch.data.nbytes] = batch.data
    return PacketBatch(buf.array[: batch.data.nbytes], batch.offsets, batch.caplens, batch.linktype), buf


def device_count() -> int:
    n = C.c_int(0)
    abi.check(abi.load_engine().pcppx_device_count(C.byref(n)), "pcppx_device_count")
    return n.value


def to_device(batch: PacketBatch, device: str = "cuda:0"):
    """Copy a host batch into HBM as torch tensors: (data u8, offsets i64-as-u64, caplens i32-as-u32)."""
    import torch

    data = torch.from_numpy(batch.data).to(device)
    offsets = torch.from_numpy(batch.offsets.view(np.int64)).to(device)
    caplens = torch.from_numpy(batch.caplens.view(np.int32)).to(device)
    return data, offsets, caplens


def records_from_device(summary_t, layers_t, n: int, max_layers: int):
    s = summary_t.cpu().numpy().view(abi.SUMMARY_DTYPE)[:n]
    if layers_t is None or max_layers == 0:
        return s, np.zeros((n, 0), dtype=abi.LAYER_DTYPE)
    lay = layers_t.cpu().numpy().view(abi.LAYER_DTYPE)[: n * max_layers].reshape(n, max_layers)
    return s, lay


def parse_on_device_ex(eng: Engine, batch: PacketBatch, opts: abi.Opts | None = None, device: str = "cuda:0",
                       summary: bool = True, tuples: bool = False, proto_stats: bool = False, flow_keys: bool = False,
                       brief: bool = False):
    """parse_on_device with the optional outputs: {"summary", "brief" (16-B pcppx_brief), "layers" (FIXED
    [n, max_layers], decoded when the layout is PACKED, through the summary or else the brief), "packed" (the raw PACKED
    entries), "tuples", "proto_stats" (dict), "flow_keys" (u32 hash5)}."""
    import torch

    opts = opts or abi.make_opts()
    data, offsets, caplens = to_device(batch, device)
    n = batch.n
    st = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device) if summary else None
    lay = torch.zeros(max(n * opts.max_layers, 1) * 8, dtype=torch.uint8, device=device)
    tp = torch.zeros(max(n, 1) * 48, dtype=torch.uint8, device=device) if tuples else None
    ps = torch.zeros(abi.PROTO_STATS, dtype=torch.int64, device=device) if proto_stats else None
    fk = torch.zeros(max(n, 1), dtype=torch.int32, device=device) if flow_keys else None
    br = torch.zeros(max(n, 1) * 16, dtype=torch.uint8, device=device) if brief else None
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, st, lay if opts.max_layers else None,
                     torch.cuda.current_stream(device).cuda_stream, flow_keys=fk, tuples=tp, proto_stats=ps, brief=br)
    torch.cuda.synchronize(device)
    out = {}
    if st is not None:
        out["summary"] = st.cpu().numpy().view(abi.SUMMARY_DTYPE)[:n]
    if br is not None:
        out["brief"] = br.cpu().numpy().view(abi.BRIEF_DTYPE)[:n]
    if opts.max_layers and (st is not None or br is not None):
        raw = lay.cpu().numpy().view(abi.LAYER_DTYPE)[: n * opts.max_layers]
        if opts.layout == abi.LAYOUT_PACKED:
            out["packed"] = raw
            out["layers"] = abi.unpack_layers(out["summary"] if st is not None else out["brief"], raw, opts.max_layers)
        else:
            out["layers"] = raw.reshape(n, opts.max_layers)
    if tp is not None:
        out["tuples"] = tp.cpu().numpy().view(abi.TUPLE_DTYPE)[:n]
    if fk is not None:
        out["flow_keys"] = fk.cpu().numpy().view(np.uint32)[:n]
    if ps is not None:
        v = ps.cpu().numpy()
        out["proto_stats"] = {f: int(v[k]) for k, f in enumerate(abi.PROTO_STATS_FIELDS)}
        out["proto_stats_raw"] = v
    return out


def parse_on_device(eng: Engine, batch: PacketBatch, opts: abi.Opts | None = None, device: str = "cuda:0"):
    """Copy a host batch to HBM, run the device-resident parse, copy the records back."""
    import torch

    opts = opts or abi.make_opts()
    data, offsets, caplens = to_device(batch, device)
    n = batch.n
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * opts.max_layers, 1) * 8, dtype=torch.uint8, device=device)
    stream = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, stream)
    torch.cuda.synchronize(device)
    return records_from_device(summary, layers, n, opts.max_layers)


def select_on_device(eng: Engine, batch: PacketBatch, keep=None, flags=None, flags_any: int = 0, invert: bool = False,
                     snaplen: int = 0, data_cap: int | None = None, max_packets: int | None = None,
                     index_only: bool = False, device: str = "cuda:0"):
    """Copy a host batch to HBM, gather the selected packets there (pcppx_select_device), copy the result back:
    (PacketBatch of the written packets, index u32 = their source packet numbers, totals dict).
    keep: n-byte mask (non-zero = selected), or flags: the batch's summary / brief record array (abi.SUMMARY_DTYPE /
    abi.BRIEF_DTYPE) tested with flags_any. data_cap / max_packets default to the batch's bytes / packets.
    index_only: no bytes move (the returned batch's data is empty, its offsets the would-be positions).
    timestamps_ns and frame_lens follow the packets through index."""
    import torch

    if (keep is None) == (flags is None):
        raise ValueError("give exactly one of keep and flags")
    n = batch.n
    data, offsets, caplens = to_device(batch, device)
    if keep is not None:
        sel_t = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(device)
        spec = abi.make_select_spec(keep=abi.ptr(sel_t) if n else 1, invert=invert, snaplen=snaplen)
    else:
        rec = np.ascontiguousarray(flags)
        if rec.dtype.itemsize not in (abi.BRIEF_DTYPE.itemsize, abi.SUMMARY_DTYPE.itemsize):
            raise ValueError("flags must be a summary or a brief record array")
        sel_t = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(device)
        spec = abi.make_select_spec(flags=(abi.ptr(sel_t) if n else 0) + abi.FLAGS_OFFSET,
                                    flags_stride=rec.dtype.itemsize, flags_any=flags_any, invert=invert, snaplen=snaplen)
    cap = int(batch.caplens.sum(dtype=np.uint64)) if data_cap is None else data_cap
    mp = n if max_packets is None else max_packets
    out_data = None if index_only else torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    out_off = torch.empty(max(mp, 1), dtype=torch.int64, device=device)
    out_cap = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_idx = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    totals = torch.empty(abi.SEL_TOTALS, dtype=torch.int64, device=device)
    eng.select_device(data, offsets, caplens, n, batch.linktype, spec, out_off, out_cap, totals, mp, out_data, cap,
                      out_idx, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    tot = abi.totals_dict(totals.cpu().numpy().view(np.uint64))
    w, wb = tot["written_packets"], tot["written_bytes"]
    index = out_idx[:w].cpu().numpy().view(np.uint32)
    out = PacketBatch(np.zeros(0, np.uint8) if index_only else out_data[:wb].cpu().numpy(),
                      out_off[:w].cpu().numpy().view(np.uint64), out_cap[:w].cpu().numpy().view(np.uint32),
                      batch.linktype)
    if batch.timestamps_ns is not None:
        out.timestamps_ns = batch.timestamps_ns[index]
    if batch.frame_lens is not None:
        out.frame_lens = batch.frame_lens[index]
    return out, index, tot


def steer_on_device(eng: Engine, batch: PacketBatch, bucket=None, key=None, key_field: str = "hash5",
                    n_buckets: int = 1, snaplen: int = 0, data_cap: int | None = None, max_packets: int | None = None,
                    index_only: bool = False, device: str = "cuda:0"):
    """Copy a host batch to HBM, steer its packets there into n_buckets packed sub-batches (pcppx_steer_device), copy
    the result back: (PacketBatch of the steered packets, bucket-major and stable; index u32 = their source packet
    numbers; bucket_first u32[n_buckets + 1]; bucket_pos u64[n_buckets + 1]; totals dict).
    bucket: n-byte column (a value >= n_buckets drops the packet), or key: a summary / brief / tuple record array
    (abi.SUMMARY_DTYPE / BRIEF_DTYPE / TUPLE_DTYPE or any structured array with key_field, a 32-bit field: "hash5",
    "hash2", "ip_key" ...) or a plain u32 column; the bucket is key % n_buckets. data_cap / max_packets default to the
    batch's bytes / packets (always enough). All or nothing: when totals["overflow"] is set the returned batch and
    index are empty and bucket_first / bucket_pos hold the sizes to call again with. index_only: no bytes move (the
    returned batch's data is empty, its offsets the would-be positions). timestamps_ns and frame_lens follow the
    packets through index (bucket_batch() keeps them per bucket)."""
    import torch

    if (bucket is None) == (key is None):
        raise ValueError("give exactly one of bucket and key")
    n = batch.n
    data, offsets, caplens = to_device(batch, device)
    if bucket is not None:
        rule_t = torch.from_numpy(np.ascontiguousarray(bucket, dtype=np.uint8)).to(device)
        spec = abi.make_steer_spec(bucket=abi.ptr(rule_t) if n else 4, n_buckets=n_buckets, snaplen=snaplen)
    else:
        rec = np.ascontiguousarray(key)
        if rec.dtype.names is None:
            if rec.dtype.itemsize != 4:
                raise ValueError("a plain key column must be 32-bit")
            field_off = 0
        else:
            ft, field_off = rec.dtype.fields[key_field][:2]
            if ft.itemsize != 4:
                raise ValueError(f"{key_field} is not a 32-bit field")
        rule_t = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(device)
        spec = abi.make_steer_spec(key=(abi.ptr(rule_t) if n else 4) + field_off, key_stride=rec.dtype.itemsize,
                                   n_buckets=n_buckets, snaplen=snaplen)
    cap = int(batch.caplens.sum(dtype=np.uint64)) if data_cap is None else data_cap
    mp = n if max_packets is None else max_packets
    out_data = None if index_only else torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    out_off = torch.empty(max(mp, 1), dtype=torch.int64, device=device)
    out_cap = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_idx = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    first = torch.empty(n_buckets + 1, dtype=torch.int32, device=device)
    pos = torch.empty(n_buckets + 1, dtype=torch.int64, device=device)
    totals = torch.empty(abi.STEER_TOTALS, dtype=torch.int64, device=device)
    eng.steer_device(data, offsets, caplens, n, batch.linktype, spec, out_off, out_cap, first, pos, totals, mp,
                     out_data, cap, out_idx, torch.cuda.current_stream(device).cuda_stream)
    torch.cuda.synchronize(device)
    tot = abi.steer_totals_dict(totals.cpu().numpy().view(np.uint64))
    w, wb = (0, 0) if tot["overflow"] else (tot["steered_packets"], tot["steered_bytes"])
    index = out_idx[:w].cpu().numpy().view(np.uint32)
    out = PacketBatch(np.zeros(0, np.uint8) if index_only else out_data[:wb].cpu().numpy(),
                      out_off[:w].cpu().numpy().view(np.uint64), out_cap[:w].cpu().numpy().view(np.uint32),
                      batch.linktype)
    if batch.timestamps_ns is not None:
        out.timestamps_ns = batch.timestamps_ns[index]
    if batch.frame_lens is not None:
        out.frame_lens = batch.frame_lens[index]
    return out, index, first.cpu().numpy().view(np.uint32), pos.cpu().numpy().view(np.uint64), tot


def tcpstream_on_device(eng: Engine, batch: PacketBatch, records, layers, info, base_clear: bool = True,
                        max_segments: int = 0, data_cap: int | None = None, max_streams: int | None = None,
                        index_only: bool = False, device: str = "cuda:0"):
    """Copy a host batch and its parse to HBM, reassemble there the TCP connection sides that are clean inside the
    batch (pcppx_tcpstream_device), copy the result back: (data u8 = the stream bytes back to back; streams =
    abi.TCPSTREAM_DTYPE records, one per clean side, ordered by the side's first packet; disposition u8[n] = abi.TCPS_*
    per source packet; seg_stream / seg_pos u32[n]; totals dict). records: the batch's summary or brief record array;
    layers: its FIXED [n, max_layers] layer array; info: its abi.REASM_DTYPE array (Engine.parse_reasm_device gives all
    three in one pass). data_cap / max_streams default to the batch's bytes / packets and max_segments to n (always
    enough). All or nothing: when totals["overflow"] is set the returned arrays are empty. The packets with
    disposition abi.TCPS_LEFT are what the caller's host TcpReassembly (or tcpstream.Reassembler) is fed."""
    import torch

    n = batch.n
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize not in (abi.BRIEF_DTYPE.itemsize, abi.SUMMARY_DTYPE.itemsize):
        raise ValueError("records must be a summary or a brief record array")
    lay = np.ascontiguousarray(layers)
    ml = lay.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)  # noqa: E731
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
    data, offsets, caplens = to_device(batch, device)
    rec_t, lay_t, info_t = up(pad(rec)), up(pad(lay.reshape(-1))), up(pad(np.ascontiguousarray(info)))
    cap = int(batch.caplens.sum(dtype=np.uint64)) if data_cap is None else data_cap
    ms = n if max_streams is None else max_streams
    out_data = None if index_only else torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    streams = torch.empty(max(ms, 1) * abi.TCPSTREAM_DTYPE.itemsize, dtype=torch.uint8, device=device)
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    seg_stream = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    seg_pos = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    totals = torch.empty(abi.TCPS_TOTALS, dtype=torch.int64, device=device)
    is_brief = rec.dtype.itemsize == abi.BRIEF_DTYPE.itemsize
    eng.tcpstream_device(data, offsets, caplens, n, batch.linktype, lay_t, ml, info_t,
                         abi.make_tcpstream_spec(base_clear, max_segments), streams, totals, ms, out_data, cap, disp,
                         seg_stream, seg_pos, torch.cuda.current_stream(device).cuda_stream,
                         summary=None if is_brief else rec_t, brief=rec_t if is_brief else None)
    torch.cuda.synchronize(device)
    tot = abi.tcpstream_totals_dict(totals.cpu().numpy().view(np.uint64))
    w, wb, k = (0, 0, 0) if tot["overflow"] else (tot["streams"], tot["bytes"], n)
    out = np.zeros(0, np.uint8) if index_only else out_data[:wb].cpu().numpy()
    recs = streams[:w * abi.TCPSTREAM_DTYPE.itemsize].cpu().numpy().view(abi.TCPSTREAM_DTYPE)
    return (out, recs, disp[:k].cpu().numpy(), seg_stream[:k].cpu().numpy().view(np.uint32),
            seg_pos[:k].cpu().numpy().view(np.uint32), tot)


def defrag6_on_device(eng: Engine, batch: PacketBatch, records, layers, info, passthrough: bool = True,
                      max_fragments: int = 0, families: int = abi.DEFRAG_FAM_V4 | abi.DEFRAG_FAM_V6,
                      data_cap: int | None = None, max_packets: int | None = None, index_only: bool = False,
                      device: str = "cuda:0"):
    """defrag_on_device through pcppx_defrag6_device: the fragment groups of the families named (abi.DEFRAG_FAM_* bits)
    are reassembled, the IPv6 ones too. Arguments and results are defrag_on_device's."""
    return defrag_on_device(eng, batch, records, layers, info, passthrough, max_fragments, data_cap, max_packets,
                            index_only, device, families)


def defrag_on_device(eng: Engine, batch: PacketBatch, records, layers, info, passthrough: bool = True,
                     max_fragments: int = 0, data_cap: int | None = None, max_packets: int | None = None,
                     index_only: bool = False, device: str = "cuda:0", families: int | None = None):
    """Copy a host batch and its parse to HBM, reassemble there the IPv4 fragment groups that are complete inside the
    batch (pcppx_defrag_device), copy the result back: (PacketBatch of the output packets in source order; index u32 =
    their source packet numbers, a reassembled packet's being the completing fragment's; first u32 = the packet whose
    headers and timestamp each carries; frags u8 = fragments merged, 0 for a copied packet; disposition u8[n] =
    abi.DEFRAG_* per source packet; totals dict).
    records: the batch's summary or brief record array; layers: its FIXED [n, max_layers] layer array; info: its
    abi.REASM_DTYPE array (Engine.parse_reasm_device gives all three in one pass). passthrough: copy every packet that
    is not merged (IPDefragUtil's output), else only the reassembled packets come out. data_cap / max_packets default
    to the batch's bytes / packets and max_fragments to n (always enough). All or nothing: when totals["overflow"] is
    set the returned batch and columns are empty. timestamps_ns follow the packets through first, frame_lens through
    index (a reassembled packet's frame length is its own length). families: None, or the abi.DEFRAG_FAM_* bits for
    pcppx_defrag6_device (defrag6_on_device)."""
    import torch

    n = batch.n
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize not in (abi.BRIEF_DTYPE.itemsize, abi.SUMMARY_DTYPE.itemsize):
        raise ValueError("records must be a summary or a brief record array")
    lay = np.ascontiguousarray(layers)
    ml = lay.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)  # noqa: E731
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
    data, offsets, caplens = to_device(batch, device)
    rec_t, lay_t, info_t = up(pad(rec)), up(pad(lay.reshape(-1))), up(pad(np.ascontiguousarray(info)))
    cap = int(batch.caplens.sum(dtype=np.uint64)) if data_cap is None else data_cap
    mp = n if max_packets is None else max_packets
    out_data = None if index_only else torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    out_off = torch.empty(max(mp, 1), dtype=torch.int64, device=device)
    out_cap = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_idx = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_first = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_frags = torch.empty(max(mp, 1), dtype=torch.uint8, device=device)
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    totals = torch.empty(abi.DEFRAG_TOTALS, dtype=torch.int64, device=device)
    is_brief = rec.dtype.itemsize == abi.BRIEF_DTYPE.itemsize
    if families is None:
        call, spec = eng.defrag_device, abi.make_defrag_spec(passthrough, max_fragments)
    else:
        call, spec = eng.defrag6_device, abi.make_defrag6_spec(passthrough, max_fragments, families)
    call(data, offsets, caplens, n, batch.linktype, lay_t, ml, info_t, spec, out_off, out_cap, totals, mp, out_data, cap,
         out_idx, out_first, out_frags, disp, torch.cuda.current_stream(device).cuda_stream,
         summary=None if is_brief else rec_t, brief=rec_t if is_brief else None)
    torch.cuda.synchronize(device)
    tot = abi.defrag_totals_dict(totals.cpu().numpy().view(np.uint64))
    w, wb = (0, 0) if tot["overflow"] else (tot["out_packets"], tot["out_bytes"])
    index = out_idx[:w].cpu().numpy().view(np.uint32)
    first = out_first[:w].cpu().numpy().view(np.uint32)
    frags = out_frags[:w].cpu().numpy()
    out = PacketBatch(np.zeros(0, np.uint8) if index_only else out_data[:wb].cpu().numpy(),
                      out_off[:w].cpu().numpy().view(np.uint64), out_cap[:w].cpu().numpy().view(np.uint32),
                      batch.linktype)
    if batch.timestamps_ns is not None:
        out.timestamps_ns = batch.timestamps_ns[first]
    if batch.frame_lens is not None:
        out.frame_lens = np.where(frags != 0, out.caplens, batch.frame_lens[index]).astype(np.uint32)
    dispo = np.zeros(0, np.uint8) if tot["overflow"] else disp[:n].cpu().numpy()
    return out, index, first, frags, dispo, tot


def frag6_on_device(eng: Engine, batch: PacketBatch, records, layers, frag_size: int = 0, mtu: int = 0,
                    families: int = abi.FRAG_FAM_V4 | abi.FRAG_FAM_V6, ids=None, id_base: int = 0, keep=None,
                    copy_rest: bool = True, honor_df: bool = False, data_cap: int | None = None,
                    max_packets: int | None = None, index_only: bool = False, device: str = "cuda:0"):
    """frag_on_device through pcppx_frag6_device: the packets of the families named (abi.FRAG_FAM_* bits) are split,
    the IPv6 ones too. ids: one u32 fragment id per source packet (None: id_base + i). The other arguments and the
    results are frag_on_device's."""
    return _frag_on_device(eng, batch, records, layers, frag_size=frag_size, mtu=mtu, keep=keep, copy_rest=copy_rest,
                           honor_df=honor_df, data_cap=data_cap, max_packets=max_packets, index_only=index_only,
                           device=device, families=families, ids=ids, id_base=id_base)


def frag_on_device(eng: Engine, batch: PacketBatch, records, layers, frag_size: int = 0, mtu: int = 0, keep=None,
                   copy_rest: bool = True, honor_df: bool = False, data_cap: int | None = None,
                   max_packets: int | None = None, index_only: bool = False, device: str = "cuda:0"):
    """Copy a host batch and its parse to HBM, split its IPv4 packets into fragments there (pcppx_frag_device), copy
    the result back: (PacketBatch of the output packets in source order, a split packet's fragments in its place; index
    u32 = their source packet numbers; frag_no u16 = the fragment's number, 0 for a copied packet; disposition u8[n] =
    abi.FRAG_* per source packet; totals dict).
    records: the batch's summary or brief record array; layers: its FIXED [n, max_layers] layer array. frag_size
    (IPFragUtil's -s) or mtu, one of them; keep: a mask of the packets to consider (None: all; IPFragUtil's -f / -d
    filters); copy_rest: copy every packet that is not split (IPFragUtil's -a), else only fragments come out. data_cap
    / max_packets default to what an index-only call says the output needs. All or nothing: when totals["overflow"] is
    set the returned batch and columns are empty. timestamps_ns follow the packets through index; a fragment's frame
    length is its caplen, a copied packet keeps its own."""
    return _frag_on_device(eng, batch, records, layers, frag_size=frag_size, mtu=mtu, keep=keep, copy_rest=copy_rest,
                           honor_df=honor_df, data_cap=data_cap, max_packets=max_packets, index_only=index_only,
                           device=device, families=None, ids=None, id_base=0)


def _frag_on_device(eng: Engine, batch: PacketBatch, records, layers, *, frag_size, mtu, keep, copy_rest, honor_df,
                    data_cap, max_packets, index_only, device, families, ids, id_base):
    """frag_on_device (families None: pcppx_frag_device) and frag6_on_device (the abi.FRAG_FAM_* bits, ids / id_base)."""
    import torch

    n = batch.n
    rec = np.ascontiguousarray(records)
    if rec.dtype.itemsize not in (abi.BRIEF_DTYPE.itemsize, abi.SUMMARY_DTYPE.itemsize):
        raise ValueError("records must be a summary or a brief record array")
    lay = np.ascontiguousarray(layers)
    ml = lay.shape[1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)  # noqa: E731
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)  # noqa: E731
    data, offsets, caplens = to_device(batch, device)
    rec_t, lay_t = up(pad(rec)), up(pad(lay.reshape(-1)))
    keep_t = None if keep is None else up(pad(np.ascontiguousarray(keep).astype(np.uint8)))
    keep_p = None if keep_t is None else abi.ptr(keep_t)
    if families is None:
        frag_call, spec = eng.frag_device, abi.make_frag_spec(frag_size, mtu, keep_p, copy_rest, honor_df)
    else:
        ids_t = None if ids is None else up(pad(np.ascontiguousarray(ids).astype(np.uint32)))
        frag_call = eng.frag6_device
        spec = abi.make_frag6_spec(frag_size, mtu, families, None if ids_t is None else abi.ptr(ids_t), id_base,
                                   keep_p, copy_rest, honor_df)
    is_brief = rec.dtype.itemsize == abi.BRIEF_DTYPE.itemsize
    st = torch.cuda.current_stream(device).cuda_stream
    totals = torch.empty(abi.FRAG_TOTALS, dtype=torch.int64, device=device)
    one64, one32 = torch.empty(1, dtype=torch.int64, device=device), torch.empty(1, dtype=torch.int32, device=device)

    def call(out_off, out_cap, mp, out_data=None, cap=0, idx=None, no=None, cnt=None, disp=None):
        frag_call(data, offsets, caplens, n, batch.linktype, lay_t, ml, spec, out_off, out_cap, totals, mp,
                  out_data, cap, idx, no, cnt, disp, st, summary=None if is_brief else rec_t,
                  brief=rec_t if is_brief else None)
        torch.cuda.synchronize(device)
        return abi.frag_totals_dict(totals.cpu().numpy().view(np.uint64))

    if data_cap is None or max_packets is None:  # the sizing call: index-only, no room, so only the totals are written
        need = call(one64, one32, 0)
        data_cap = need["out_bytes"] if data_cap is None else data_cap
        max_packets = need["out_packets"] if max_packets is None else max_packets
    cap, mp = data_cap, max_packets
    out_data = None if index_only else torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    out_off = torch.empty(max(mp, 1), dtype=torch.int64, device=device)
    out_cap = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_idx = torch.empty(max(mp, 1), dtype=torch.int32, device=device)
    out_no = torch.empty(max(mp, 1), dtype=torch.int16, device=device)
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(out_off, out_cap, mp, out_data, cap, out_idx, out_no, None, disp)
    w, wb = (0, 0) if tot["overflow"] else (tot["out_packets"], tot["out_bytes"])
    index = out_idx[:w].cpu().numpy().view(np.uint32)
    frag_no = out_no[:w].cpu().numpy().view(np.uint16)
    dispo = np.zeros(0, np.uint8) if tot["overflow"] else disp[:n].cpu().numpy()
    out = PacketBatch(np.zeros(0, np.uint8) if index_only else out_data[:wb].cpu().numpy(),
                      out_off[:w].cpu().numpy().view(np.uint64), out_cap[:w].cpu().numpy().view(np.uint32),
                      batch.linktype)
    if batch.timestamps_ns is not None:
        out.timestamps_ns = batch.timestamps_ns[index]
    if batch.frame_lens is not None:
        split = dispo[index] == abi.FRAG_SPLIT if w else np.zeros(0, bool)
        out.frame_lens = np.where(split, out.caplens, batch.frame_lens[index]).astype(np.uint32)
    return out, index, frag_no, dispo, tot


def tlsfp_on_device(eng: Engine, batch: PacketBatch, client: bool = True, server: bool = True,
                    opts: abi.Opts | None = None, want_text: bool = True, device: str = "cuda:0"):
    """Copy a host batch to HBM, parse it there and fingerprint its TLS hellos (pcppx_tlsfp_device) without the records
    leaving the device in between; copy the result back: (recs abi.TLSFP_REC_DTYPE[k] in source order, text u8 = the
    fingerprint texts back to back (empty with want_text = False), tuples abi.TUPLE_DTYPE[n] = the parse's 5-tuple
    extracts that recs["index"] indexes, disposition u8[n] = abi.TLSFP_* per source packet, totals dict). The buffers
    are sized by a first call with max_recs = 0, which overflows and writes the totals alone."""
    import torch

    opts = opts or abi.make_opts()
    n, ml = batch.n, opts.max_layers
    data, offsets, caplens = to_device(batch, device)
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * ml, 1) * 8, dtype=torch.uint8, device=device)
    tuples = torch.zeros(max(n, 1) * 48, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, st, tuples=tuples)
    spec = abi.make_tlsfp_spec(client, server)
    totals = torch.empty(abi.TLSFP_TOTALS, dtype=torch.int64, device=device)

    def call(recs, max_recs, text=None, cap=0, disp=None):
        eng.tlsfp_device(data, offsets, caplens, n, batch.linktype, layers, ml, spec, recs, totals, max_recs, text, cap,
                         disp, st, summary=summary)
        torch.cuda.synchronize(device)
        return abi.tlsfp_totals_dict(totals.cpu().numpy().view(np.uint64))

    need = call(torch.empty(40, dtype=torch.uint8, device=device), 0)
    k, nb = need["client_n"] + need["server_n"], need["text_bytes"]
    recs = torch.empty(max(k, 1) * 40, dtype=torch.uint8, device=device)
    text = torch.empty(max(nb, 1), dtype=torch.uint8, device=device) if want_text else None
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(recs, k, text, nb, disp)
    assert tot["overflow"] == 0
    return (recs.cpu().numpy().view(abi.TLSFP_REC_DTYPE)[:k], text[:nb].cpu().numpy() if want_text else
            np.zeros(0, np.uint8), tuples.cpu().numpy().view(abi.TUPLE_DTYPE)[:n], disp[:n].cpu().numpy(), tot)


def dns_on_device(eng: Engine, batch: PacketBatch, sections: int = 15, opts: abi.Opts | None = None,
                  want_names: bool = True, device: str = "cuda:0"):
    """Copy a host batch to HBM, parse it there and walk its DNS messages (pcppx_dns_device) without the records leaving
    the device in between; copy the result back: (msgs abi.DNS_MSG_DTYPE[m] in source order, rrs abi.DNS_RR_DTYPE[k]
    message by message, names u8 = the decoded names back to back (empty with want_names = False), disposition u8[n] =
    abi.DNS_* per source packet, totals dict). The buffers are sized by a first call without room, which overflows and
    writes the totals alone."""
    import torch

    opts = opts or abi.make_opts()
    n, ml = batch.n, opts.max_layers
    data, offsets, caplens = to_device(batch, device)
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * ml, 1) * 8, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, st)
    spec = abi.make_dns_spec(sections)
    totals = torch.empty(abi.DNS_TOTALS, dtype=torch.int64, device=device)

    def call(msgs, max_msgs, rrs, max_rrs, names=None, cap=0, disp=None):
        eng.dns_device(data, offsets, caplens, n, batch.linktype, layers, ml, spec, msgs, rrs, totals, max_msgs,
                       max_rrs, names, cap, disp, st, summary=summary)
        torch.cuda.synchronize(device)
        return abi.dns_totals_dict(totals.cpu().numpy().view(np.uint64))

    one = torch.empty(40, dtype=torch.uint8, device=device)
    need = call(one, 0, one, 0)
    m, k, nb = need["msgs"], need["rrs"], need["name_bytes"]
    msgs = torch.empty(max(m, 1) * 40, dtype=torch.uint8, device=device)
    rrs = torch.empty(max(k, 1) * 32, dtype=torch.uint8, device=device)
    names = torch.empty(max(nb, 1), dtype=torch.uint8, device=device) if want_names else None
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(msgs, m, rrs, k, names, nb, disp)
    assert tot["overflow"] == 0
    return (msgs.cpu().numpy().view(abi.DNS_MSG_DTYPE)[:m], rrs.cpu().numpy().view(abi.DNS_RR_DTYPE)[:k],
            names[:nb].cpu().numpy() if want_names else np.zeros(0, np.uint8), disp[:n].cpu().numpy(), tot)


def http_on_device(eng: Engine, batch: PacketBatch, spec: abi.HttpSpec | None = None, opts: abi.Opts | None = None,
                   want_text: bool = True, device: str = "cuda:0"):
    """Copy a host batch to HBM, parse it there and walk its HTTP messages (pcppx_http_device) without the records
    leaving the device in between; copy the result back: (msgs abi.HTTP_MSG_DTYPE[m] in source order, fields
    abi.HTTP_FIELD_DTYPE[k] message by message, text u8 = the bytes spec asks for back to back (empty with want_text =
    False), disposition u8[n] = abi.HTTP_* per source packet, totals dict). spec None: every field, the first line's
    text. The buffers are sized by a first call without room, which overflows and writes the totals alone."""
    import torch

    opts = opts or abi.make_opts()
    spec = spec or abi.make_http_spec((), abi.HTTP_FIELDS_ALL, abi.HTTP_TEXT_FIRST_LINE)
    n, ml = batch.n, opts.max_layers
    data, offsets, caplens = to_device(batch, device)
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * ml, 1) * 8, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, st)
    totals = torch.empty(abi.HTTP_TOTALS, dtype=torch.int64, device=device)

    def call(msgs, max_msgs, fields, max_fields, text=None, cap=0, disp=None):
        eng.http_device(data, offsets, caplens, n, batch.linktype, layers, ml, spec, msgs, fields, totals, max_msgs,
                        max_fields, text, cap, disp, st, summary=summary)
        torch.cuda.synchronize(device)
        return abi.http_totals_dict(totals.cpu().numpy().view(np.uint64))

    one = torch.empty(48, dtype=torch.uint8, device=device)
    need = call(one, 0, one, 0)
    m, k, nb = need["msgs"], need["fields"], need["text_bytes"]
    msgs = torch.empty(max(m, 1) * 48, dtype=torch.uint8, device=device)
    fields = torch.empty(max(k, 1) * 24, dtype=torch.uint8, device=device)
    text = torch.empty(max(nb, 1), dtype=torch.uint8, device=device) if want_text else None
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(msgs, m, fields, k, text, nb, disp)
    assert tot["overflow"] == 0
    return (msgs.cpu().numpy().view(abi.HTTP_MSG_DTYPE)[:m], fields.cpu().numpy().view(abi.HTTP_FIELD_DTYPE)[:k],
            text[:nb].cpu().numpy() if want_text else np.zeros(0, np.uint8), disp[:n].cpu().numpy(), tot)


def ssl_on_device(eng: Engine, batch: PacketBatch, kinds: int = 3, opts: abi.Opts | None = None,
                  want_names: bool = True, device: str = "cuda:0"):
    """Copy a host batch to HBM, parse it there and walk its SSL/TLS records (pcppx_ssl_device) without the records
    leaving the device in between; copy the result back: (msgs abi.SSL_MSG_DTYPE[m] in source order, hellos
    abi.SSL_HELLO_DTYPE[k] message by message, names u8 = the SNI host names back to back (empty with want_names =
    False), hash5 u32[n] = the parse's flow keys (what pcapplusplus_amd.ssl.analyze keys flows by), disposition u8[n] =
    abi.SSL_* per source packet, totals dict). The buffers are sized by a first call without room, which overflows and
    writes the totals alone."""
    import torch

    opts = opts or abi.make_opts()
    spec = abi.make_ssl_spec(kinds)
    n, ml = batch.n, opts.max_layers
    data, offsets, caplens = to_device(batch, device)
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * ml, 1) * 8, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, st)
    totals = torch.empty(abi.SSL_TOTALS, dtype=torch.int64, device=device)

    def call(msgs, max_msgs, hellos, max_hellos, names=None, cap=0, disp=None):
        eng.ssl_device(data, offsets, caplens, n, batch.linktype, layers, ml, spec, msgs, hellos, totals, max_msgs,
                       max_hellos, names, cap, disp, st, summary=summary)
        torch.cuda.synchronize(device)
        return abi.ssl_totals_dict(totals.cpu().numpy().view(np.uint64))

    one = torch.empty(32, dtype=torch.uint8, device=device)
    need = call(one, 0, one, 0)
    m, k, nb = need["msgs"], need["hellos"], need["name_bytes"]
    msgs = torch.empty(max(m, 1) * 32, dtype=torch.uint8, device=device)
    hellos = torch.empty(max(k, 1) * 32, dtype=torch.uint8, device=device)
    names = torch.empty(max(nb, 1), dtype=torch.uint8, device=device) if want_names else None
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(msgs, m, hellos, k, names, nb, disp)
    assert tot["overflow"] == 0
    hash5 = summary.cpu().numpy().view(abi.SUMMARY_DTYPE)[:n]["hash5"].copy()
    return (msgs.cpu().numpy().view(abi.SSL_MSG_DTYPE)[:m], hellos.cpu().numpy().view(abi.SSL_HELLO_DTYPE)[:k],
            names[:nb].cpu().numpy() if want_names else np.zeros(0, np.uint8), hash5, disp[:n].cpu().numpy(), tot)


def sip_on_device(eng: Engine, batch: PacketBatch, spec: abi.SipSpec | None = None, opts: abi.Opts | None = None,
                  want_text: bool = True, device: str = "cuda:0"):
    """Copy a host batch to HBM, parse it there and walk its SIP messages (pcppx_sip_device) without the records
    leaving the device in between; copy the result back: (msgs abi.SIP_MSG_DTYPE[m] in source order, fields
    abi.SIP_FIELD_DTYPE[k] message by message, sdps abi.SIP_SDP_DTYPE[s] in message order, text u8 = the bytes spec
    asks for back to back (empty with want_text = False), disposition u8[n] = abi.SIP_* per source packet, totals
    dict). spec None: Call-ID, From, To and CSeq with their values and the first line's text. The buffers are sized by
    a first call without room, which overflows (where there is a message) and writes the totals alone."""
    import torch

    opts = opts or abi.make_opts()
    spec = spec or abi.make_sip_spec()
    n, ml = batch.n, opts.max_layers
    data, offsets, caplens = to_device(batch, device)
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * ml, 1) * 8, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, st)
    totals = torch.empty(abi.SIP_TOTALS, dtype=torch.int64, device=device)

    def call(msgs, max_msgs, fields, max_fields, sdps, max_sdps, text=None, cap=0, disp=None):
        eng.sip_device(data, offsets, caplens, n, batch.linktype, layers, ml, spec, msgs, fields, sdps, totals,
                       max_msgs, max_fields, max_sdps, text, cap, disp, st, summary=summary)
        torch.cuda.synchronize(device)
        return abi.sip_totals_dict(totals.cpu().numpy().view(np.uint64))

    one = torch.empty(48, dtype=torch.uint8, device=device)
    need = call(one, 0, one, 0, one, 0)
    m, k, ns, nb = need["msgs"], need["fields"], need["sdps"], need["text_bytes"]
    msgs = torch.empty(max(m, 1) * 48, dtype=torch.uint8, device=device)
    fields = torch.empty(max(k, 1) * 24, dtype=torch.uint8, device=device)
    sdps = torch.empty(max(ns, 1) * 32, dtype=torch.uint8, device=device)
    text = torch.empty(max(nb, 1), dtype=torch.uint8, device=device) if want_text else None
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(msgs, m, fields, k, sdps, ns, text, nb, disp)
    assert tot["overflow"] == 0
    return (msgs.cpu().numpy().view(abi.SIP_MSG_DTYPE)[:m], fields.cpu().numpy().view(abi.SIP_FIELD_DTYPE)[:k],
            sdps.cpu().numpy().view(abi.SIP_SDP_DTYPE)[:ns],
            text[:nb].cpu().numpy() if want_text else np.zeros(0, np.uint8), disp[:n].cpu().numpy(), tot)


def dhcp_on_device(eng: Engine, batch: PacketBatch, spec: abi.DhcpSpec | None = None, opts: abi.Opts | None = None,
                   want_values: bool = True, device: str = "cuda:0"):
    """Copy a host batch to HBM, parse it there and walk its DHCP / DHCPv6 messages (pcppx_dhcp_device) without the
    records leaving the device in between; copy the result back: (msgs abi.DHCP_MSG_DTYPE[m] in source order, options
    abi.DHCP_OPTION_DTYPE[k] message by message, values u8 = the value bytes spec asks for back to back (empty with
    want_values = False), disposition u8[n] = abi.DHCP_* per source packet, totals dict). spec None: the asset
    discovery options (abi.DHCP_ASSET_CODES4 / 6) with their values. The buffers are sized by a first call without
    room, which overflows (where there is a message) and writes the totals alone."""
    import torch

    opts = opts or abi.make_opts()
    spec = spec or abi.make_dhcp_spec()
    n, ml = batch.n, opts.max_layers
    data, offsets, caplens = to_device(batch, device)
    summary = torch.zeros(max(n, 1) * 32, dtype=torch.uint8, device=device)
    layers = torch.zeros(max(n * ml, 1) * 8, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    eng.parse_device(data, offsets, caplens, n, batch.linktype, opts, summary, layers, st)
    totals = torch.empty(abi.DHCP_TOTALS, dtype=torch.int64, device=device)

    def call(msgs, max_msgs, options, max_options, values=None, cap=0, disp=None):
        eng.dhcp_device(data, offsets, caplens, n, batch.linktype, layers, ml, spec, msgs, options, totals, max_msgs,
                        max_options, values, cap, disp, st, summary=summary)
        torch.cuda.synchronize(device)
        return abi.dhcp_totals_dict(totals.cpu().numpy().view(np.uint64))

    one = torch.empty(80, dtype=torch.uint8, device=device)
    need = call(one, 0, one, 0)
    m, k, nb = need["msgs"], need["options"], need["value_bytes"]
    msgs = torch.empty(max(m, 1) * 80, dtype=torch.uint8, device=device)
    options = torch.empty(max(k, 1) * 16, dtype=torch.uint8, device=device)
    values = torch.empty(max(nb, 1), dtype=torch.uint8, device=device) if want_values else None
    disp = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    tot = call(msgs, m, options, k, values, nb, disp)
    assert tot["overflow"] == 0
    return (msgs.cpu().numpy().view(abi.DHCP_MSG_DTYPE)[:m], options.cpu().numpy().view(abi.DHCP_OPTION_DTYPE)[:k],
            values[:nb].cpu().numpy() if want_values else np.zeros(0, np.uint8), disp[:n].cpu().numpy(), tot)


def bpf_on_device(eng: Engine, batch: PacketBatch, programs, frame_lens=None, device: str = "cuda:0"):
    """Copy a host batch to HBM, run the classic BPF programs over its packets there (pcppx_bpf_device), copy the
    verdicts back: (matched u8[n], bucket u8[n] = the first accepting program or 0xFF, ret u32[n] = its return value,
    totals dict). programs: 1..16 programs in load order (pcapplusplus_amd.bpf); frame_lens: u32 wire lengths for
    LD|LEN (None: the batch's frame_lens if it has them, else the caplens)."""
    import torch

    n = batch.n
    if frame_lens is None:
        frame_lens = batch.frame_lens
    data, offsets, caplens = to_device(batch, device)
    fl = None if frame_lens is None else \
        torch.from_numpy(np.ascontiguousarray(frame_lens, dtype=np.uint32).view(np.int32)).to(device)
    matched = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    bucket = torch.empty(max(n, 1), dtype=torch.uint8, device=device)
    ret = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    totals = torch.empty(abi.BPF_TOTALS, dtype=torch.int64, device=device)
    with eng.bpf_load(programs) as flt:
        eng.bpf_device(flt, data, offsets, caplens, n, batch.linktype, totals, matched, bucket, ret, fl,
                       torch.cuda.current_stream(device).cuda_stream)
        torch.cuda.synchronize(device)
    return (matched[:n].cpu().numpy(), bucket[:n].cpu().numpy(), ret[:n].cpu().numpy().view(np.uint32),
            abi.bpf_totals_dict(totals.cpu().numpy().view(np.uint64)))


def bucket_batch(out: PacketBatch, bucket_first, b: int) -> PacketBatch:
    """Bucket b of a steered batch as a PacketBatch view (no copy): the same data, the bucket's rows of offsets /
    caplens (and of timestamps_ns / frame_lens, which followed the packets through index)."""
    lo, hi = int(bucket_first[b]), int(bucket_first[b + 1])
    cut = lambda a: None if a is None else a[lo:hi]  # noqa: E731
    return PacketBatch(out.data, out.offsets[lo:hi], out.caplens[lo:hi], out.linktype, cut(out.timestamps_ns),
                       cut(out.frame_lens))
