// pcppx_internal.h — kernel launchers shared by the C-ABI layer (not part of the public ABI).
#pragma once

#include <hip/hip_runtime.h>

#include "pcppx.h"

namespace pcppx
{
int check_launch(const char* what, hipStream_t stream);
// wave_stats: null, or parse_waves(n) 16-B per-wave collectStats records, summed by launch_proto_stats_reduce
// win_stats: null, or the context's two 64-bit counters: a window sample (window_sample_kernel: ~64 tiles' live and
// deep-stack packets) runs ahead of the parse on the same stream and adds to them
int launch_parse(const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r, hipStream_t stream,
                 void* wave_stats = nullptr, unsigned long long* win_stats = nullptr);
uint32_t parse_waves(uint32_t n);
int launch_proto_stats_reduce(const void* wave_stats, uint32_t n, uint64_t* out, hipStream_t stream);
int launch_filter(const pcppx_batch* b, const pcppx_records* r, uint32_t ml, const pcppx_match_spec* spec,
                  uint64_t seq_base, uint64_t* keys, uint64_t* first, uint32_t capacity, uint8_t* matched,
                  pcppx_packet_stats* stats, hipStream_t stream);
// the partitioned flow table (product): queues = P x rec_cap 16-B records, fill = P zeroed counters
uint32_t flow_partitions(uint32_t capacity);
uint32_t flow_queue_capacity(uint32_t n, uint32_t capacity);
int launch_flow_count_part(const pcppx_summary* sum, const uint32_t* dkeys, const uint32_t* caplens, uint32_t n,
                           uint32_t* keys, uint64_t* packets, uint64_t* bytes, uint32_t capacity, uint64_t* stats,
                           void* queues, uint32_t rec_cap, uint32_t* fill, hipStream_t stream);
int launch_parse_reasm(const pcppx_batch* b, const pcppx_opts* o, pcppx_records* r, pcppx_reasm_info* info,
                       hipStream_t stream, void* wave_stats = nullptr, unsigned long long* win_stats = nullptr);
int launch_reasm(const pcppx_batch* b, const pcppx_records* r, uint32_t ml, pcppx_reasm_info* info, hipStream_t stream);
// PCPPX_LAYOUT_DENSE on the host path: a chunk's FIXED rows (n x ml) -> its chains back to back (dense), the chain
// lengths read from n_layers[i * nl_stride] (a summary's or a brief's byte 14); *total = the entries written.
// block_sums: dense_blocks(n) words of scratch.
uint32_t dense_blocks(uint32_t n);
int launch_dense_compact(const pcppx_layer* fixed, const uint8_t* n_layers, uint32_t nl_stride, uint32_t n, uint32_t ml,
                         pcppx_layer* dense, uint32_t* block_sums, uint32_t* total, hipStream_t stream);
// the compacted chains to page-locked host memory through its device mapping (dst_mapped), positions chained across the
// chunks of a batch on the device: *cum_out = (*base_in or 0) + *count; at_base: entries at dst_mapped + base (else + 0)
int launch_dense_push(const pcppx_layer* dense, const uint32_t* count, const uint32_t* base_in, pcppx_layer* dst_mapped,
                      bool at_base, uint32_t* cum_out, hipStream_t stream);
// pcppx_select_device (pcppx_select.hip): count, block bases and copy, three launches on `stream`. scratch:
// select_scratch_bytes(n) bytes of block sums and bases; one block gathers kSelectBlockPk packets (16 tiles).
// Arguments are checked by the caller; n > 0.
constexpr uint32_t kSelectBlockPk = 1024;
uint32_t select_blocks(uint32_t n);
uint64_t select_scratch_bytes(uint32_t n);
int launch_select(const pcppx_batch* b, const pcppx_select_spec* spec, const pcppx_selection* out, void* scratch,
                  hipStream_t stream);
// pcppx_steer_device (pcppx_steer.hip): count, per-bucket scan, bucket bases and copy, four launches on `stream`.
// scratch: steer_scratch_bytes(n, n_buckets) bytes (the block sums per bucket, bucket-major, and the bucket totals);
// one block steers kSteerBlockPk packets, a scan step takes kSteerScanStep block sums. Arguments are checked by the
// caller; n > 0.
constexpr uint32_t kSteerBlockPk = 1024;
constexpr uint32_t kSteerScanStep = 64;
uint32_t steer_blocks(uint32_t n);
uint64_t steer_scratch_bytes(uint32_t n, uint32_t n_buckets);
int launch_steer(const pcppx_batch* b, const pcppx_steer_spec* spec, const pcppx_steering* out, void* scratch,
                 hipStream_t stream);
// pcppx_defrag_device / pcppx_defrag6_device (pcppx_defrag.hip): one clear and five to seven launches on `stream`
// (collect, verdict, count, bases, place; with out->data the merge copy and the header patch); families: the
// PCPPX_DEFRAG_FAM_* bits (V4 alone: pcppx_defrag_device's kernels). scratch: defrag_scratch_bytes(n, max_fragments)
// bytes (include/pcppx.h gives the formula); one block takes kDefragBlockPk packets, the verdict / merge / patch
// kernels kDefragCandPerBlock candidates; n_layers: packet 0's n_layers byte (a summary's or a brief's), nl_stride
// bytes apart. Arguments are checked by the caller; n > 0.
constexpr uint32_t kDefragBlockPk = 1024;
constexpr uint32_t kDefragCandPerBlock = 256;
constexpr uint32_t kDefragMinSlots = 64;
uint32_t defrag_blocks(uint32_t n);
uint32_t defrag_room(uint32_t n, uint32_t max_fragments);  // F: the candidates the scratch holds
uint32_t defrag_slots(uint32_t room);                      // C: the group table's slots
uint64_t defrag_scratch_bytes(uint32_t n, uint32_t max_fragments);
int launch_defrag(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* n_layers,
                  uint32_t nl_stride, const pcppx_reasm_info* info, uint32_t max_fragments, uint32_t passthrough,
                  uint32_t families, const pcppx_defragged* out, void* scratch, hipStream_t stream);
// pcppx_tcpstream_device (pcppx_tcpstream.hip): two clears and nine launches on `stream` (collect, second sides, join,
// chain, verdict, count, bases, place, emit). scratch: tcpstream_scratch_bytes(n, max_segments) bytes (include/pcppx.h
// gives the formula); one block takes kTcpsBlockPk packets, the per-candidate kernels kTcpsCandPerBlock candidates;
// rec0: packet 0's summary or brief (hash5 at byte 0, n_layers at 14, l4_layer at 15), rec_stride bytes apart.
// Arguments are checked by the caller; n > 0.
constexpr uint32_t kTcpsBlockPk = 1024;
constexpr uint32_t kTcpsCandPerBlock = 256;
constexpr uint32_t kTcpsMinSlots = 64;
uint32_t tcpstream_room(uint32_t n, uint32_t max_segments);  // F: the candidates the scratch holds
uint32_t tcpstream_slots(uint32_t room);                     // C: the connection table's and the segment table's slots
uint64_t tcpstream_scratch_bytes(uint32_t n, uint32_t max_segments);
int launch_tcpstream(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0,
                     uint32_t rec_stride, const pcppx_reasm_info* info, const pcppx_tcpstream_spec* spec,
                     const pcppx_tcpstreams* out, void* scratch, hipStream_t stream);
// pcppx_frag_device / pcppx_frag6_device (pcppx_frag.hip): three or four launches on `stream` (plan, bases, emit; with
// out->data the header patch). spec->families = V4 alone (pcppx_frag_device's spec arrives so): frag's kernels.
// scratch: frag_scratch_bytes(n) bytes (include/pcppx.h gives the formula); one block takes kFragBlockPk source
// packets and puts out all of their output packets; n_layers / nl_stride as for launch_defrag. Arguments are checked
// by the caller; n > 0.
constexpr uint32_t kFragBlockPk = 1024;
uint32_t frag_blocks(uint32_t n);
uint64_t frag_scratch_bytes(uint32_t n);
int launch_frag(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* n_layers,
                uint32_t nl_stride, const pcppx_frag6_spec* spec, const pcppx_fragmented* out, void* scratch,
                hipStream_t stream);
// The message operators pcppx_tlsfp_device, pcppx_dns_device, pcppx_http_device, pcppx_ssl_device, pcppx_sip_device and
// pcppx_dhcp_device (pcppx_<op>.hip): three launches on `stream` each (plan, bases, emit). scratch:
// <op>_scratch_bytes(n) bytes (include/pcppx.h gives the formulas); one block takes k<Op>BlockPk source packets and writes their records; rec0:
// packet 0's summary or brief, rec_stride bytes apart. Arguments are checked by the caller; n > 0.
constexpr uint32_t kTlsfpBlockPk = 1024;
constexpr uint32_t kDnsBlockPk = 1024;
constexpr uint32_t kHttpBlockPk = 1024;
constexpr uint32_t kSslBlockPk = 1024;
constexpr uint32_t kSipBlockPk = 1024;
constexpr uint32_t kDhcpBlockPk = 1024;
uint32_t tlsfp_blocks(uint32_t n);
uint32_t dns_blocks(uint32_t n);
uint32_t http_blocks(uint32_t n);
uint32_t ssl_blocks(uint32_t n);
uint32_t sip_blocks(uint32_t n);
uint32_t dhcp_blocks(uint32_t n);
uint64_t tlsfp_scratch_bytes(uint32_t n);
uint64_t dns_scratch_bytes(uint32_t n);
uint64_t http_scratch_bytes(uint32_t n);
uint64_t ssl_scratch_bytes(uint32_t n);
uint64_t sip_scratch_bytes(uint32_t n);
uint64_t dhcp_scratch_bytes(uint32_t n);
int launch_tlsfp(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
                 const pcppx_tlsfp_spec* spec, const pcppx_tlsfps* out, void* scratch, hipStream_t stream);
int launch_dns(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
               const pcppx_dns_spec* spec, const pcppx_dns_out* out, void* scratch, hipStream_t stream);
int launch_http(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
                const pcppx_http_spec* spec, const pcppx_http_out* out, void* scratch, hipStream_t stream);
int launch_ssl(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
               const pcppx_ssl_spec* spec, const pcppx_ssl_out* out, void* scratch, hipStream_t stream);
int launch_sip(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
               const pcppx_sip_spec* spec, const pcppx_sip_out* out, void* scratch, hipStream_t stream);
int launch_dhcp(const pcppx_batch* b, const pcppx_layer* layers, uint32_t ml, const uint8_t* rec0, uint32_t rec_stride,
                const pcppx_dhcp_spec* spec, const pcppx_dhcp_out* out, void* scratch, hipStream_t stream);
// pcppx_bpf_device (pcppx_bpf.hip): one launch on `stream` (the caller has cleared out->totals on it). insns: the
// validated programs back to back in device memory; program p is insns[start[p] .. start[p + 1]); uses_mem: bit p set
// when program p loads from M[] (only then are its slots cleared). Arguments are checked by the caller; n > 0.
struct BpfPrograms
{
	const pcppx_bpf_insn* insns;
	uint32_t n_progs;
	uint32_t uses_mem;
	uint32_t start[PCPPX_BPF_MAX_PROGRAMS + 1];
};
int launch_bpf(const pcppx_batch* b, const uint32_t* frame_lens, const BpfPrograms& progs, const pcppx_bpf_verdicts* out,
               hipStream_t stream);
}  // namespace pcppx
