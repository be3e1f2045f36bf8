/*
 * pcppx.h — C ABI of the MI355X packet-dissection engine (drop-in boundary).
 *
 * This is the boundary that replaces the per-packet Packet++ parse path
 *   RawPacket -> pcpp::Packet(RawPacket*, ...)          Packet++/src/Packet.cpp:202-209, :66-196
 *   pcpp::hash5Tuple / pcpp::hash2Tuple                  Packet++/src/PacketUtils.cpp:139-245
 *   IPv4 header checksum                                 Packet++/src/IPv4Layer.cpp:410-412
 *   TcpLayer/UdpLayer::calculateChecksum(false)          Packet++/src/TcpLayer.cpp:271, UdpLayer.cpp:47
 * with one batched call over many packets that sit in GPU memory (HBM).
 *
 * Conventions:
 *   - every function returns 0 or a negative PCPPX_E* code; nothing throws across the ABI;
 *   - the caller owns every buffer; records are arrays sized n (and n*max_layers);
 *   - a context belongs to one host thread and one GPU; contexts are never shared.
 *
 * Records mirror what a pcpp::Packet exposes after parsing:
 *   pcppx_layer   <-> Layer::getProtocol/getOsiModelLayer/getData()-raw/getHeaderLen/getDataLen
 *                      (Packet++/header/Layer.h, ProtocolType.h:35-284)
 *   pcppx_summary <-> Packet::isPacketOfType (proto_mask, Packet.cpp:614-640), hash5Tuple(false/true),
 *                      hash2Tuple, the IPv4/L4 checksums.
 * Layers the engine builds: Ethernet II / 802.3 / LLC, VLAN, MPLS, IPv4, IPv6 (+ extensions), GREv0/v1,
 * PPP_PPTP, ARP, ICMP (+ the IPv4 header an error message quotes), TCP, UDP, the VXLAN and GTPv1 tunnels
 * (+ the inner packet), Payload, Trailer, the first layers of link types Ethernet, raw IP (RAW, DLT_RAW1/2,
 * IPV4, IPV6), Linux SLL / SLL2, Null/Loopback, Cisco HDLC and NFLOG (its TLVs walked to the payload record), and the first L7 layers it can name: HTTPRequest /
 * HTTPResponse (+ the Payload body), SSL records, DNS, SSH messages (port 22) and MySQL (port 3306, where no
 * dissector ahead of it in TcpLayer::parseNextLayer takes the other port).
 * Packets for which the reference would build a layer outside this scope (other L7 dissectors, IGMP, PPPoE,
 * ...) are flagged PCPPX_F_NEEDS_HOST_L7 / PCPPX_F_NEEDS_HOST_PROTO: their
 * layer prefix is exact, and the host owns the rest.
 */
#ifndef PCPPX_H
#define PCPPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCPPX_ABI_VERSION 7
/* the library is built with hidden visibility: exactly the functions declared here are exported */
#define PCPPX_API __attribute__((visibility("default")))
#define PCPPX_MAX_LAYERS 16     /* fixed depth cap; deeper chains set PCPPX_F_DEPTH_OVERFLOW */
#define PCPPX_MAX_CAPLEN 65535  /* larger packets are flagged PCPPX_F_OVERSIZE and not parsed */

/* error codes */
#define PCPPX_OK 0
#define PCPPX_E_INVAL -1    /* bad argument (null pointer, n too large, max_layers > 16 ...) */
#define PCPPX_E_NODEV -2    /* no HIP device / bad ordinal */
#define PCPPX_E_HIP -3      /* a HIP runtime call failed */
#define PCPPX_E_NOMEM -4    /* device or pinned allocation failed */
#define PCPPX_E_LINKTYPE -5 /* link type not handled by the device path */

/* pcppx_summary.flags */
#define PCPPX_F_NEEDS_HOST_L7 0x0001    /* an L4 payload would go to an L7 dissector the device does not
                                           build (TcpLayer.cpp:372-491, UdpLayer.cpp:103-178); chain stops at
                                           the L4 layer */
#define PCPPX_F_NEEDS_HOST_PROTO 0x0002 /* an out-of-scope L2/L3 layer would be built (PPPoE, IGMP, IPSec,
                                           VRRP, ICMPv6, STP, WoL); chain stops before it */
#define PCPPX_F_DEPTH_OVERFLOW 0x0004   /* more than max_layers layers; extra layers not written */
#define PCPPX_F_OVERSIZE 0x0008         /* caplen > PCPPX_MAX_CAPLEN: not parsed */
#define PCPPX_F_IP_CSUM 0x0010          /* ip_csum_* computed (an IPv4 layer exists and want_checksums) */
#define PCPPX_F_IP_CSUM_OK 0x0020       /* ip_csum_calc == ip_csum_stored */
#define PCPPX_F_L4_CSUM 0x0040          /* l4_csum_* computed (a TCP/UDP layer exists and want_checksums) */
#define PCPPX_F_L4_CSUM_OK 0x0080       /* l4_csum_calc == l4_csum_stored */
#define PCPPX_F_TRAILER 0x0100          /* last layer is a PacketTrailer (Packet.cpp:178-195) */
#define PCPPX_F_BAD_DESC 0x0200         /* offsets[i] + caplens[i] > batch data_len: not parsed */
/* The first L7 layer of a NEEDS_HOST_L7 packet, where the device can name it (the content checks of
 * TcpLayer.cpp:372-415 / UdpLayer.cpp:103-116 it restates): with PCPPX_F_L7_KNOWN set, the packet's chain holds
 * an HTTPRequest/HTTPResponse, SSL or DNS layer exactly when the matching bit is set, i.e.
 * Packet::isPacketOfType(HTTP / SSL / DNS) is decided. Not set for tunnels (VXLAN, GTPv1) whose inner packet only
 * the host parses (the VXLAN / GTPv1 tunnels the device builds itself are not NEEDS_HOST_L7). An HTTP / SSL /
 * DNS layer the device builds itself is in the records and proto_mask instead, with none of these bits: the
 * packet is not NEEDS_HOST_L7. */
#define PCPPX_F_L7_KNOWN 0x0400
#define PCPPX_F_L7_HTTP 0x0800
#define PCPPX_F_L7_SSL 0x1000
#define PCPPX_F_L7_DNS 0x2000
#define PCPPX_F_NEEDS_HOST \
	(PCPPX_F_NEEDS_HOST_L7 | PCPPX_F_NEEDS_HOST_PROTO | PCPPX_F_OVERSIZE | PCPPX_F_BAD_DESC)

/* One parsed layer, 8 bytes. */
typedef struct pcppx_layer {
	uint8_t proto;     /* pcpp::ProtocolType (ProtocolType.h:42-258) */
	uint8_t osi;       /* pcpp::OsiModelLayer (ProtocolType.h:266-284) */
	uint16_t offset;   /* Layer::getData() - RawPacket::getRawData() */
	uint16_t hdr_len;  /* Layer::getHeaderLen() */
	uint16_t data_len; /* Layer::getDataLen() */
} pcppx_layer;

/* Per-packet summary, 32 bytes. */
typedef struct pcppx_summary {
	uint32_t hash5;          /* pcpp::hash5Tuple(&packet, false) */
	uint32_t hash5_dir;      /* pcpp::hash5Tuple(&packet, true) */
	uint32_t hash2;          /* pcpp::hash2Tuple(&packet) */
	uint16_t flags;          /* PCPPX_F_* */
	uint8_t n_layers;        /* layers in the chain (capped at max_layers, see PCPPX_F_DEPTH_OVERFLOW) */
	uint8_t l4_layer;        /* index of the layer hash5Tuple takes its ports from (last TCP, else last
	                            UDP); 0xFF if none */
	uint64_t proto_mask;     /* bit p set iff some layer has protocol p: Packet::isPacketOfType(p) */
	uint16_t ip_csum_calc;   /* computeChecksum over the first IPv4 header, checksum field zeroed
	                            (IPv4Layer.cpp:410-412) — the value computeCalculateFields would store */
	uint16_t ip_csum_stored; /* be16 of the header's checksum field */
	uint16_t l4_csum_calc;   /* {Tcp,Udp}Layer::calculateChecksum(false) of layer l4_layer */
	uint16_t l4_csum_stored; /* be16 of that layer's checksum field */
} pcppx_summary;

/* The summary's first 16 bytes alone (ABI 7): what a caller that reads the layer records needs besides them. The
 * protocol mask is the OR of the recorded chain's protocols (pcppx_chain_proto_mask below: exact when the chain is
 * recorded whole -- no PCPPX_F_DEPTH_OVERFLOW and n_layers <= max_layers), and the checksum verdicts are the flags
 * (PCPPX_F_IP_CSUM[_OK], PCPPX_F_L4_CSUM[_OK]); only the computed / stored checksum values are not carried. */
typedef struct pcppx_brief {
	uint32_t hash5;     /* = pcppx_summary.hash5 */
	uint32_t hash5_dir; /* = pcppx_summary.hash5_dir */
	uint32_t hash2;     /* = pcppx_summary.hash2 */
	uint16_t flags;     /* = pcppx_summary.flags */
	uint8_t n_layers;   /* = pcppx_summary.n_layers */
	uint8_t l4_layer;   /* = pcppx_summary.l4_layer */
} pcppx_brief;

/* A batch of packets: bytes of packet i are data[offsets[i] .. offsets[i] + caplens[i]).
 * For the fast path packets should be stored back to back in ascending offset order (any order and
 * gaps are legal; they only cost bandwidth). */
typedef struct pcppx_batch {
	const uint8_t* data;
	const uint64_t* offsets;
	const uint32_t* caplens;
	uint64_t data_len; /* bytes addressable at data (bounds every packet) */
	uint32_t n;
	uint16_t linktype; /* pcpp::LinkLayerType (RawPacket.h:24-178) for every packet of the batch */
	uint16_t reserved;
} pcppx_batch;

/* pcpp::PacketParseOptions (Packet++/header/Packet.h:17-37) plus output selection. */
typedef struct pcppx_opts {
	uint32_t parse_until_family; /* pcpp::ProtocolTypeFamily; 0 = UnknownProtocol (parse everything) */
	uint8_t parse_until_osi;     /* pcpp::OsiModelLayer; 8 = OsiModelLayerUnknown */
	uint8_t want_checksums;      /* compute IPv4 / L4 checksums */
	uint8_t max_layers;          /* 0 = do not write layers; else layers stride per packet (1..16) */
	uint8_t window;              /* PCPPX_WINDOW_*: the header window the parse gathers per packet (a speed choice for
	                                the caller's traffic: the records are identical whichever window runs) */
	uint8_t layout;              /* PCPPX_LAYOUT_*: how pcppx_records.layers is laid out */
	uint8_t reserved[3];
} pcppx_opts;
#define PCPPX_WINDOW_DEFAULT 0 /* the engine's choice (ABI 7), from the traffic this context has parsed with it: ahead
                                  of those parses (each until the first decision, then one in 16) ~64 tiles of the batch
                                  count their deep stacks (a sampling kernel: after up to two VLAN tags an MPLS label,
                                  or an IP layer not followed by TCP / UDP); when more than 1 in 256 sampled packets
                                  had one, the next launches run as DEEP (checksum launches) / with the second round
                                  (parse-only), otherwise checksum launches gather one 96-B window (5 waves/SIMD) and
                                  parse-only ones run as SHORT. Until 2048 packets were sampled: one 96-B window for checksum launches,
                                  96 B + a second round up to 144 B for parse-only ones. pcppx_window_choice() */
#define PCPPX_WINDOW_DEEP 1    /* checksum launches too gather the two-round 144-B window: deep stacks stay on the
                                  fast path instead of the generic walk; 4 waves/SIMD. Parse-only: as DEFAULT */
#define PCPPX_WINDOW_SHORT 2   /* parse-only launches: one 96-B gather round and no second one (7 KiB of LDS per wave
                                  instead of 10: more waves per CU) -- faster on plain Eth / VLAN / IP / L4 traffic
                                  (IMIX 7%, 64-B packets 16%), about 2x slower on deep encapsulation, whose stacks past
                                  96 B take the generic walk. Checksum launches: as DEFAULT */

/* pcppx_records.layers layouts (pcppx_opts.layout). Both hold the same pcppx_layer entries, bit for bit:
 *   FIXED:  packet i's layer k is layers[i * max_layers + k], k < min(n_layers, max_layers); the entries of a row past
 *           its chain are unspecified (the fast path stores whole rows, zero past the chain; the generic walk stores
 *           the chain alone: a reused buffer keeps what it held there). Nothing is written outside rows 0 .. n-1.
 *   PACKED: the chains densely per 64-packet tile: the entries of tile t (packets 64t .. 64t+63) start at
 *           layers[64 * t * max_layers], and packet i's entries follow those of the packets
 *           before it in its tile: layers[64 * t * max_layers + sum_{64t <= j < i} min(n_layers_j, max_layers) + k].
 *           A tile writes only inside its own region, entries [64 * t * max_layers, min(64 * (t + 1), n) * max_layers):
 *           the run of its first total_t = sum_j min(n_layers_j, max_layers) entries holds the chains, and the rest of
 *           the region is unspecified (a packet off the fast path first stores its chain at its FIXED slot inside the
 *           region, from where the run is packed: such entries at or past the run keep those values). Nothing is
 *           written at or past layers[n * max_layers].
 *           The buffer is sized as for FIXED (n * max_layers entries); the summary or the brief is required (its
 *           n_layers decode the positions: pcppx_unpack_layers[_brief] below, pcppx::unpackLayers in include/pcppx.hpp). The write
 *           traffic is the chain, not max_layers rows per packet. max_layers <= PCPPX_PACKED_MAX_LAYERS. Device parse
 *           only; the consumers of a parse's records (pcppx_filter_device, pcppx_reasm_device) read FIXED records and
 *           refuse PACKED ones (pcppx_records.layout). */
#define PCPPX_LAYOUT_FIXED 0
#define PCPPX_LAYOUT_PACKED 1
#define PCPPX_PACKED_MAX_LAYERS 12
/*   DENSE (ABI 7, host path): the chains back to back over the whole batch, in packet order: packet i's entries are
 *           layers[sum_{j < i} min(n_layers_j, max_layers) + k]; pcppx_records.layers_written returns the total. The
 *           buffer must hold the total (n * max_layers entries always do; unwritten memory is never touched), and
 *           only the chains cross PCIe (config 3: 4.2 entries = 34 B per packet instead of 8 * max_layers).
 *           max_layers <= PCPPX_MAX_LAYERS. pcppx_parse_batch_host only. Entry positions are 32-bit: a batch with
 *           n * max_layers > UINT32_MAX is refused with PCPPX_E_INVAL (split it; 268M packets at max_layers 16). */
#define PCPPX_LAYOUT_DENSE 2

/* The 5-tuple extract (the compact record of the bandwidth runs), 48 bytes per packet: exactly the
 * fields pcpp::hash5Tuple reads (Packet++/src/PacketUtils.cpp:139-210), from the same layers as the summary's
 * hashes -- the first IPv4 layer, else the first IPv6 layer (getLayerOfType<IPv4Layer>() / <IPv6Layer>()), and
 * the last TCP layer, else the last UDP layer (getLayerOfType<TcpLayer>(true) / <UdpLayer>(true)). */
typedef struct pcppx_tuple {
	uint8_t src_ip[16]; /* IPv4: getSrcIPv4Address() bytes in packet order, then 12 zero bytes; IPv6: ipSrc; none: 0 */
	uint8_t dst_ip[16];
	uint16_t src_port;  /* the port layer's getSrcPort() (host order); 0 without a TCP/UDP layer */
	uint16_t dst_port;  /* getDstPort() */
	uint8_t ip_version; /* 4 or 6: which layer the addresses come from; 0 = no IP layer */
	uint8_t ip_proto;   /* that layer's protocol (IPv4) / nextHeader (IPv6) byte: hash5Tuple's last byte */
	uint8_t l4_proto;   /* pcpp::TCP (4) / pcpp::UDP (5): the port layer; 0 = none */
	uint8_t has_5tuple; /* 1 iff hash5Tuple hashes these fields: an IP layer, a TCP/UDP layer and no ICMP layer
	                       (PacketUtils.cpp:141-148); 0: hash5 == 0 */
	uint32_t hash5;     /* pcpp::hash5Tuple(&packet, false) (= pcppx_summary.hash5) */
	uint16_t flags;     /* pcppx_summary.flags (PCPPX_F_NEEDS_HOST*: the fields of a flagged packet are those of the
	                       chain prefix the device built) */
	uint8_t n_layers;   /* pcppx_summary.n_layers */
	uint8_t reserved;
} pcppx_tuple;

/* PacketStats::collectStats (Examples/DpdkExample-FilterTraffic/Common.h:83-104) over a parsed batch: word k of
 * pcppx_records.proto_stats (device memory, PCPPX_PROTO_STATS words, accumulated by += across calls) counts */
#define PCPPX_PS_PACKETS 0    /* packets of the batch */
#define PCPPX_PS_ETH 1        /* isPacketOfType(Ethernet) */
#define PCPPX_PS_ARP 2        /* isPacketOfType(ARP) */
#define PCPPX_PS_IPV4 3       /* isPacketOfType(IPv4) */
#define PCPPX_PS_IPV6 4       /* isPacketOfType(IPv6) */
#define PCPPX_PS_TCP 5        /* isPacketOfType(TCP) */
#define PCPPX_PS_UDP 6        /* isPacketOfType(UDP) */
#define PCPPX_PS_HTTP 7       /* isPacketOfType(HTTP), over the packets the device settles (below) */
#define PCPPX_PS_DNS 8        /* isPacketOfType(DNS), the same */
#define PCPPX_PS_SSL 9        /* isPacketOfType(SSL) (collectStats' tlsCount), the same */
#define PCPPX_PS_NEEDS_HOST 10 /* packets whose HTTP/DNS/SSL answer the host must complete: a chain stopped before an
                                 out-of-scope layer (NEEDS_HOST_PROTO), a bad record, or an L7 payload the device could
                                 not classify -- as pcppx_packet_stats.needs_host_count */
#define PCPPX_PROTO_STATS 16  /* words (11-15 are zero) */

/* Output arrays (same memory space as the batch for the _device call, host for the _host call). The device writes them
 * with vector stores, so every array must have its record's natural alignment: 16 bytes for summary, brief, tuples
 * and pcppx_reasm_info, 8 bytes for layers and proto_stats, 4 bytes for flow_keys. Only entries 0 .. n-1 of an array
 * (n * max_layers entries of layers) are written, every byte of them except the unspecified layer entries of
 * pcppx_opts.layout; proto_stats is accumulated. */
typedef struct pcppx_records {
	pcppx_summary* summary; /* n entries, or NULL when `brief` is set; may also be NULL on the device path when max_layers
	                           is 0 and one of tuples / flow_keys / proto_stats is set (e.g. a flow table's launch: dense
	                           keys + collectStats) */
	pcppx_layer* layers;    /* n * max_layers entries in pcppx_opts.layout, or NULL when max_layers == 0 */
	uint32_t* flow_keys;    /* optional (NULL): n entries, flow_keys[i] = summary[i].hash5 -- the dense column
	                           FilterTraffic's flow table is keyed by (pcppx_flow_count_keys_device reads 8 B per
	                           packet from it and caplens instead of 36 B through the summary) */
	pcppx_tuple* tuples;    /* optional (NULL): n 5-tuple extracts. Device path only */
	uint64_t* proto_stats;  /* optional (NULL): PCPPX_PROTO_STATS counters, accumulated (collectStats). Device path
	                           only; calls that set it on one context are ordered (they share its scratch) */
	uint8_t layout;         /* PCPPX_LAYOUT_* of `layers`: written by the parse calls (= opts->layout); read by
	                           pcppx_filter_device / pcppx_reasm_device, which refuse PCPPX_LAYOUT_PACKED records.
	                           Zero-initialised records are FIXED. */
	uint8_t reserved[7];
	pcppx_brief* brief;     /* optional (NULL), ABI 7: n 16-B briefs (the summary's first half), beside or instead of
	                           the summary -- the record a layer-reading caller needs (device and host paths) */
	uint64_t layers_written; /* out: layer entries written (PCPPX_LAYOUT_DENSE: the total of the chains) */
} pcppx_records;

/* Packet::isPacketOfType's mask (bit p for every protocol p of the chain) from a packet's recorded layers: equals
 * pcppx_summary.proto_mask when the chain is recorded whole (pcppx_brief) */
static inline uint64_t pcppx_chain_proto_mask(const pcppx_layer* chain, unsigned n_layers)
{
	uint64_t m = 0;
	for (unsigned k = 0; k < n_layers; ++k)
		m |= chain[k].proto < 64 ? 1ull << chain[k].proto : 0ull;
	return m;
}

/* The caller's own host parse of ONE packet — its Packet++ (`pcpp::Packet packet(&raw, parseUntil...)`) turned
 * into this engine's records: summary + up to opts->max_layers layers, as the engine would write them had it
 * finished the chain. The engine never calls it and libpcppx.so never links Packet++: the C++ facade
 * (pcppx.hpp, Engine::setHostParser) calls it for packets flagged PCPPX_F_NEEDS_HOST, so that a caller's
 * per-packet loop sees every packet completely. INTEGRATION.md §2 has an implementation over pcpp::Packet.
 * Returns 0 or a negative PCPPX_E_* code. */
typedef int (*pcppx_host_parse_fn)(const uint8_t* packet, uint32_t caplen, uint16_t linktype, const pcppx_opts* opts,
                                   pcppx_summary* summary, pcppx_layer* layers);

typedef struct pcppx_ctx pcppx_ctx;

/* library / device management */
PCPPX_API int pcppx_abi_version(void);
PCPPX_API const char* pcppx_strerror(int err);
PCPPX_API int pcppx_device_count(int* out);
PCPPX_API int pcppx_runtime_info(int device, char* buf, size_t len); /* HIP runtime/driver versions, device name */
PCPPX_API int pcppx_open(int device_ordinal, pcppx_ctx** out); /* one per host thread & GPU */
PCPPX_API void pcppx_close(pcppx_ctx* ctx);
PCPPX_API int pcppx_sync(pcppx_ctx* ctx);                      /* wait for everything queued on ctx's stream */
PCPPX_API void* pcppx_ctx_stream(pcppx_ctx* ctx);              /* the context's own hipStream_t */
/* the window a PCPPX_WINDOW_DEFAULT launch with / without checksums would run with now (waits for the last sample) */
PCPPX_API int pcppx_window_choice(pcppx_ctx* ctx, int want_checksums, int* window);
PCPPX_API void pcppx_default_opts(pcppx_opts* opts);           /* Packet(RawPacket*) defaults + checksums + 16 layers */

/* Device-resident parse. batch and records hold device pointers; the kernels are queued on
 * hip_stream (a hipStream_t; NULL = the null/default stream, as everywhere in HIP) and the call returns
 * without waiting. pcppx_ctx_stream() gives the context's own non-blocking stream. */
PCPPX_API int pcppx_parse_batch_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_opts* opts,
                             pcppx_records* out, void* hip_stream);

/* Host-to-host parse: batch and records hold host pointers. The context stages the bytes through pinned
 * buffers in chunks, overlapping H2D copies, kernels and D2H copies; returns when out is filled. The FIXED or the DENSE
 * layout; a summary and / or a brief; records.tuples and records.proto_stats must be NULL (device-path outputs). */
PCPPX_API int pcppx_parse_batch_host(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_opts* opts,
                           pcppx_records* out);

/* Per-flow counters keyed by hash5Tuple (Examples/DpdkExample-FilterTraffic/AppWorkerThread.h:99-125).
 * Device pointers: summary[n] from a previous parse, caplens[n]. The table is open-addressed with
 * `capacity` slots (power of two), split into min(512, max(1, capacity / 4096)) equal regions by the key's hash (a
 * flow lives in its region; every region has at least 4096 slots, or is the whole table); keys[i]==0 marks an
 * empty slot — flow key 0 (non-5-tuple packets, PacketUtils.cpp:141-148) is counted in stats[0] (packets) /
 * stats[1] (bytes) instead, and packets whose region had no free slot in stats[2]. Counts accumulate across
 * calls; calls on one context are ordered (they share its scratch). HBM scratch held by the context: record
 * queues of 16 B x min(n, 2^24) x ~1.25 (grown in stream order, freed by pcppx_close).
 * stats is three words: key-0 packets, key-0 bytes, lost packets; nothing behind stats[2] is touched.
 * Slots with key 0 keep zero counts: packets[s] == bytes[s] == 0 wherever keys[s] == 0.
 * caplens[i] <= PCPPX_MAX_CAPLEN is required wherever the key is non-zero (a launch carries a flow's bytes in a
 * 40-bit field: 2^24 - 1 packets of 65535 B at most). Records of a parse satisfy it: OVERSIZE and BAD_DESC packets
 * have key 0, and key-0 bytes are summed in 64 bits whatever the caplen. With larger values the per-flow counts are
 * unspecified.
 * A call of more than 2^24 - 1 packets is processed in consecutive launches with the same result. */
/* The same over the dense key column a parse wrote (pcppx_records.flow_keys): keys_in[i] = hash5 of packet i. */
PCPPX_API int pcppx_flow_count_keys_device(pcppx_ctx* ctx, const uint32_t* keys_in, const uint32_t* caplens, uint32_t n,
                                           uint32_t* keys, uint64_t* packets, uint64_t* bytes, uint32_t capacity,
                                           uint64_t* stats, void* hip_stream);
PCPPX_API int pcppx_flow_count_device(pcppx_ctx* ctx, const pcppx_summary* summary, const uint32_t* caplens,
                            uint32_t n, uint32_t* keys, uint64_t* packets, uint64_t* bytes,
                            uint32_t capacity, uint64_t* stats, void* hip_stream);

/* ---- DpdkExample-FilterTraffic's worker on the device ----
 * PacketMatchingEngine::isMatched (Examples/DpdkExample-FilterTraffic/PacketMatchingEngine.h:43-107),
 * the matched-flow table keyed by hash5Tuple and PacketStats::collectStats (AppWorkerThread.h:85-139,
 * Common.h:83-104), over a parsed device batch (records from pcppx_parse_batch_device; max_layers >= 1).
 * Packet order is the worker's receive order: packet i of the batch has sequence number seq_base + i,
 * and a packet matches if it matches on its own or an earlier packet of the same 5-tuple flow matched.
 * The flow table (flow_keys / flow_first, `capacity` slots, power of two, zero-initialised) persists
 * across batches like the worker's m_FlowTable. A used slot holds flow_keys[s] = 1 << 32 | hash5 and flow_first[s] =
 * ~(sequence number of the flow's first packet that matched on its own); seq_base + n must stay below 2^64 - 1
 * (sequence number 2^64 - 1 would be stored as 0, the empty value). */
typedef struct pcppx_match_spec {
	uint32_t src_ip;   /* IPv4Address::toInt() (network byte order in memory); 0 = any */
	uint32_t dst_ip;   /* 0 = any */
	uint16_t src_port; /* host order; 0 = any */
	uint16_t dst_port; /* 0 = any */
	uint8_t protocol;  /* pcpp::TCP (4) or pcpp::UDP (5); anything else = any */
	uint8_t reserved[3];
} pcppx_match_spec;

typedef struct pcppx_packet_stats { /* PacketStats, Examples/DpdkExample-FilterTraffic/Common.h:57-142 */
	uint64_t packet_count, eth_count, arp_count, ipv4_count, ipv6_count, tcp_count, udp_count;
	uint64_t http_count, dns_count, tls_count; /* isPacketOfType(HTTP / DNS / SSL) of the packets the device
	                                              settles: the first L7 layer of a NEEDS_HOST_L7 packet is
	                                              classified on the device (TcpLayer.cpp:372-415,
	                                              UdpLayer.cpp:103-116) */
	uint64_t matched_tcp_flows, matched_udp_flows, matched_packets;
	uint64_t needs_host_count;                  /* packets whose counters the host must complete: chains stopped
	                                              before an out-of-scope L2/L3 layer (NEEDS_HOST_PROTO), bad
	                                              records, or UDP tunnels (VXLAN, GTPv1) carrying inner packets */
	uint64_t flow_table_full;                   /* matched packets whose flow found no free slot in the device flow
	                                              table (capacity too small for the traffic's flows): the reference's
	                                              unordered_map never fills, so when this is non-zero the
	                                              matched_* counters and verdicts are no longer the reference's */
} pcppx_packet_stats;

PCPPX_API int pcppx_filter_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                        const pcppx_match_spec* spec, uint64_t seq_base, uint64_t* flow_keys, uint64_t* flow_first,
                        uint32_t capacity, uint8_t* matched, pcppx_packet_stats* stats, void* hip_stream);

/* The same worker over host batches, with the flow table, packet sequence and statistics held by the
 * context (one context = one worker, AppWorkerThread.h:45-162): packets are staged to HBM, parsed and
 * filtered there; matched[i] = 1 for packets the worker would send on (AppWorkerThread.h:127-131).
 * *stats (may be NULL) receives the statistics accumulated since the last pcppx_filter_reset.
 * pcppx_filter_reset sizes (capacity: power of two, 0 = 4M slots) and clears the flow table; the first
 * pcppx_filter_batch_host call does it implicitly. */
PCPPX_API int pcppx_filter_reset(pcppx_ctx* ctx, uint32_t capacity);
PCPPX_API int pcppx_filter_batch_host(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_match_spec* spec,
                            uint8_t* matched, pcppx_packet_stats* stats);

/* ---- reassembly front ends ----
 * The stateless per-packet half of the two reassemblers, over a parsed device batch:
 *   IPReassembly::processPacket up to its fragment-table lookup (Packet++/src/IPReassembly.cpp:281-322):
 *     non-IP / non-fragment / malformed classification, the fragment key hashPacket() (FNV-1 over src, dst,
 *     IP id: IPReassembly.cpp:103-115 for IPv4, :190-205 for IPv6), getFragmentId / getFragmentOffset and
 *     isFirstFragment / isLastFragment (IPv4Layer.cpp:415-438, IPv6Extensions.cpp:71-91);
 *   TcpReassembly::reassemblePacket up to its connection lookup (Packet++/src/TcpReassembly.cpp:81-141):
 *     non-IP / non-TCP / no-data classification, the TCP payload size and SYN/FIN/RST; the connection key
 *     is hash5Tuple = pcppx_summary.hash5 (TcpReassembly.cpp:141).
 * The stateful tables (fragment lists, connection map, callbacks) stay with the host caller.
 * A packet whose chain the engine did not finish (PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC,
 * DEPTH_OVERFLOW, or NEEDS_HOST_L7 on a UDP payload) gets *_HOST unless its first IPv4 layer is recorded
 * (then ip_status is exact). NEEDS_HOST_L7 on a TCP payload is exact: the dissectors reached from TCP ports
 * (TcpLayer.cpp:372-491) build no further IP or TCP layer. */
#define PCPPX_IPR_NON_IP 0       /* IPReassembly::NON_IP_PACKET */
#define PCPPX_IPR_NON_FRAGMENT 1 /* IPReassembly::NON_FRAGMENT */
#define PCPPX_IPR_MALFORMED 2    /* IPReassembly::MALFORMED_FRAGMENT (payload size > data len, :315-320) */
#define PCPPX_IPR_FRAGMENT 3     /* a fragment: ip_key / frag_id / frag_offset set; the host table decides */
#define PCPPX_IPR_HOST 15        /* the packet's chain is not finished on the device: the host decides */
#define PCPPX_IPR_F_FIRST 0x10   /* isFirstFragment() */
#define PCPPX_IPR_F_LAST 0x20    /* isLastFragment() */
#define PCPPX_IPR_F_IPV6 0x40    /* the IPv6 wrapper was used (no IPv4 layer in the packet); a fragment header
                                    lies inside the IPv6 header, which a non-malformed fragment holds whole */

#define PCPPX_TCPR_NON_IP 0  /* TcpReassembly::NonIpPacket */
#define PCPPX_TCPR_NON_TCP 1 /* TcpReassembly::NonTcpPacket */
#define PCPPX_TCPR_NO_DATA 2 /* TcpReassembly::Ignore_PacketWithNoData */
#define PCPPX_TCPR_DATA 3    /* goes on to the connection table keyed by hash5 */
#define PCPPX_TCPR_HOST 15   /* the packet's chain is not finished on the device: the host decides */
#define PCPPX_TCPR_F_FIN 0x10
#define PCPPX_TCPR_F_SYN 0x20
#define PCPPX_TCPR_F_RST 0x40

typedef struct pcppx_reasm_info { /* 16 bytes per packet */
	uint32_t ip_key;      /* hashPacket() when ip_status is PCPPX_IPR_FRAGMENT, else 0 */
	uint32_t frag_id;     /* getFragmentId(): be16 IPv4 id / be32 IPv6 fragment id (0 unless a fragment) */
	uint16_t frag_offset; /* getFragmentOffset() in bytes (0 unless a fragment) */
	uint8_t ip_status;    /* PCPPX_IPR_* (low nibble) | PCPPX_IPR_F_* */
	uint8_t tcp_status;   /* PCPPX_TCPR_* (low nibble) | PCPPX_TCPR_F_* of the last TCP layer */
	uint32_t tcp_payload; /* the last TCP layer's getLayerPayloadSize() (0 without a TCP layer) */
} pcppx_reasm_info;

/* batch (device pointers) + its records from pcppx_parse_batch_device (max_layers >= 1, the same
 * max_layers here) -> info[n] (device). Queued on hip_stream; returns without waiting. */
PCPPX_API int pcppx_reasm_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                       pcppx_reasm_info* info, void* hip_stream);

/* pcppx_parse_batch_device and pcppx_reasm_device in one pass: the parse kernel writes info[n] too, from the
 * header bytes it already holds (no second read of the packets or records). opts->max_layers >= 1. The
 * records and info equal those of the two calls made one after the other. */
PCPPX_API int pcppx_parse_batch_device_reasm(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_opts* opts,
                                   pcppx_records* out, pcppx_reasm_info* info, void* hip_stream);

/* ---- select: gather the kept packets of a device batch into a packed batch (the worker's send-on step) ----
 * What FilterTraffic's worker does after isMatched (sendPacketsTo->sendPacket / pcapWriter->writePacket,
 * AppWorkerThread.h:127-139), for packets that sit in HBM: a stable stream compaction of variable-length packets.
 * The packets chosen by a mask (pcppx_filter_device's matched[]) or by a flags test (a parse's summary / brief flags,
 * e.g. PCPPX_F_NEEDS_HOST: the packets the host must finish) are copied, in source order, back to back into
 * out->data, with offsets / caplens (an ordinary pcppx_batch for every other entry point) and their source packet
 * numbers. Added within ABI 7: new symbols only, no existing record or call changes (PCPPX_ABI_VERSION stays 7). */
typedef struct pcppx_select_spec {
	const uint8_t* keep;   /* device, n bytes: packet i is selected iff keep[i] != 0. NULL = flags mode */
	const void* flags;     /* flags mode: device address of packet 0's 16-bit flags word
	                          (&summary[0].flags or &brief[0].flags) */
	uint32_t flags_stride; /* bytes between consecutive packets' flags words (32 summary / 16 brief) */
	uint16_t flags_any;    /* flags mode: selected iff (flags & flags_any) != 0 */
	uint8_t invert;        /* 1: select the complement (the unmatched stream) */
	uint8_t reserved;
	uint32_t snaplen;      /* 0 = whole packet; else the output caplen is min(caplen, snaplen) */
	uint32_t reserved2;
} pcppx_select_spec;

/* pcppx_selection.totals words */
#define PCPPX_SEL_SELECTED_PACKETS 0 /* packets the rule chose whose descriptor is in bounds */
#define PCPPX_SEL_SELECTED_BYTES 1   /* their output lengths (after snaplen) */
#define PCPPX_SEL_WRITTEN_PACKETS 2  /* the prefix of them that fitted max_packets / data_cap */
#define PCPPX_SEL_WRITTEN_BYTES 3
#define PCPPX_SEL_BAD_DESC 4         /* packets the rule chose with offsets[i] + caplens[i] > data_len: never read,
                                        never selected */
#define PCPPX_SEL_TOTALS 8           /* words 5-7 zero */

typedef struct pcppx_selection { /* all device pointers */
	uint8_t* data;        /* packed bytes of the written packets, back to back, no padding; NULL = index-only */
	uint64_t data_cap;
	uint64_t* offsets;    /* max_packets entries: offsets[j] = sum of the output lengths of selected packets < j */
	uint32_t* caplens;    /* max_packets entries */
	uint32_t* index;      /* optional (NULL): index[j] = source packet number, strictly ascending */
	uint32_t max_packets;
	uint32_t reserved;
	uint64_t* totals;     /* PCPPX_SEL_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_selection;

/* Written rule: the selected packet of rank r (source order) at exclusive byte position p is written iff
 * r < max_packets and, when data != NULL, p + len <= data_cap. Both conditions are monotone, so the written packets
 * are a prefix of the selected ones; no packet is written partially. Entries offsets / caplens / index[j] for
 * j >= WRITTEN_PACKETS and bytes of data at or beyond WRITTEN_BYTES are not touched. With data == NULL (index-only)
 * no bytes move, the byte capacity is not applied and offsets hold the would-be positions. A packet of any caplen
 * (0, or above PCPPX_MAX_CAPLEN) is copied: select is not a parse; the source batch may be gapped, unordered or
 * overlapping; out->data must not overlap batch->data. Source bytes are read only through aligned 16-B granules
 * (which never cross a page) that hold at least one byte of a selected, in-bounds packet.
 * PCPPX_E_INVAL before any device work: a null ctx, batch, spec, out, totals, offsets or caplens; keep and flags both
 * null or both set; flags mode with a flags_stride other than 16 or 32; a non-zero reserved field. n == 0 is legal
 * and writes zero totals. The work is queued on hip_stream and the call returns without waiting (the totals stay on
 * the device); calls on one context are ordered (they share its scratch), as the flow-count calls are. */
PCPPX_API int pcppx_select_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_select_spec* spec,
                                  pcppx_selection* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_select_reference(const pcppx_batch* batch, const pcppx_select_spec* spec, pcppx_selection* out);

/* ---- steer: stable K-way flow steering of a device batch into packed sub-batches (what RSS does on a NIC) ----
 * FilterTraffic's worker rule (a packet matches if an earlier packet of its 5-tuple flow matched,
 * AppWorkerThread.h:99-131) is well defined across cores only because RSS hands every flow to one RX queue.
 * pcppx_steer_device is that step for packets in HBM: packet i goes to bucket[i] (column mode) or to
 * key[i] % n_buckets (key mode: a parse's hash5 / hash2 column, or a reassembly ip_key), and the packets are moved
 * bucket by bucket, each bucket in source order, into one packed batch: one radix pass of a counting sort whose
 * payload is the packet bytes; select generalised from 2 ways to K. Added within ABI 7: new symbols only. */
#define PCPPX_STEER_MAX_BUCKETS 256
typedef struct pcppx_steer_spec {
	const uint8_t* bucket; /* column mode: device, n bytes: packet i goes to bucket[i]; a value >= n_buckets means
	                          "not steered" (dropped, counted; its descriptor is not read). NULL = key mode */
	const void* key;       /* key mode: device address of packet 0's 32-bit key (&summary[0].hash5, &brief[0].hash5,
	                          &tuples[0].hash5, flow_keys, &summary[0].hash2, &info[0].ip_key ...):
	                          bucket = key % n_buckets */
	uint32_t key_stride;   /* key mode: bytes between consecutive packets' keys: a multiple of 4, 4..256; the key
	                          4-byte aligned (column mode: ignored) */
	uint32_t n_buckets;    /* 1..PCPPX_STEER_MAX_BUCKETS */
	uint32_t snaplen;      /* 0 = whole packet; else the output caplen is min(caplen, snaplen) */
	uint32_t reserved;
} pcppx_steer_spec;

/* pcppx_steering.totals words */
#define PCPPX_STEER_STEERED_PACKETS 0 /* packets with a bucket < n_buckets whose descriptor is in bounds */
#define PCPPX_STEER_STEERED_BYTES 1   /* their output lengths (after snaplen) */
#define PCPPX_STEER_DROPPED 2         /* column values >= n_buckets */
#define PCPPX_STEER_BAD_DESC 3        /* packets with a bucket whose offsets[i] + caplens[i] > data_len (or wraps 64
                                         bits): never read, never steered */
#define PCPPX_STEER_OVERFLOW 4        /* 1: the steered packets / bytes exceed max_packets / data_cap; else 0 */
#define PCPPX_STEER_TOTALS 8          /* words 5-7 zero */

typedef struct pcppx_steering { /* all device pointers */
	uint8_t* data;          /* packed bytes of the steered packets, back to back, no padding; NULL = index-only */
	uint64_t data_cap;
	uint64_t* offsets;      /* max_packets entries: offsets[r] = sum of the output lengths of output packets < r */
	uint32_t* caplens;      /* max_packets entries */
	uint32_t* index;        /* optional (NULL): index[r] = source packet number of output packet r */
	uint32_t* bucket_first; /* n_buckets + 1 entries: bucket b = output packets [bucket_first[b], bucket_first[b+1]) */
	uint64_t* bucket_pos;   /* n_buckets + 1 entries: its bytes = data[bucket_pos[b], bucket_pos[b+1]) */
	uint32_t max_packets;
	uint32_t reserved;
	uint64_t* totals;       /* PCPPX_STEER_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_steering;

/* Steered: packet i is steered iff its rule gives a bucket < n_buckets and offsets[i] + caplens[i] <= data_len (the
 * 64-bit wrap checked too). A packet with a bucket that is out of bounds is never read and counts in BAD_DESC; a column
 * value >= n_buckets counts in DROPPED (key mode drops nothing).
 * Output order: bucket-major and stable. Bucket 0's steered packets in source order, then bucket 1's, and so on, back
 * to back with no padding inside buckets or between them: offsets[r] is the sum of the output lengths of the output
 * packets before r, bucket_first[n_buckets] = STEERED_PACKETS, bucket_pos[n_buckets] = STEERED_BYTES. The whole output
 * is an ordinary pcppx_batch, and so is bucket b without a copy: the same data / data_len, offsets + bucket_first[b],
 * caplens + bucket_first[b], n = bucket_first[b+1] - bucket_first[b].
 * Capacity is all or nothing (unlike select's prefix rule: a prefix of a bucket-major output is useless): the output
 * overflows iff STEERED_PACKETS > max_packets or, when data != NULL, STEERED_BYTES > data_cap. Then OVERFLOW = 1,
 * totals / bucket_first / bucket_pos hold the full would-be values (size the buffers from them and call again) and
 * data / offsets / caplens / index are not touched at all. max_packets = n and data_cap = the sum of the caplens
 * always suffice. With data == NULL (index-only) no bytes move, the byte capacity is not applied and offsets hold the
 * would-be positions.
 * As select: a packet of any caplen (0, or above PCPPX_MAX_CAPLEN) is copied; the source batch may be gapped,
 * unordered or overlapping; out->data must not overlap batch->data. Source bytes are read only through aligned 16-B
 * granules (which never cross a page) that hold at least one byte of a steered packet. Nothing outside
 * [0, STEERED_BYTES) of data and nothing outside the first STEERED_PACKETS entries of offsets / caplens / index is
 * written. The output is a pure function of the inputs, bit-identical from run to run: every place comes from counts
 * and scans, none from the order in which atomics land.
 * PCPPX_E_INVAL before any device work: a null ctx, batch, spec, out, totals, offsets, caplens, bucket_first or
 * bucket_pos; bucket and key both null or both set; n_buckets 0 or above PCPPX_STEER_MAX_BUCKETS; key mode with a
 * key_stride that is not a multiple of 4 in 4..256 or a key that is not 4-byte aligned; a non-zero reserved field.
 * n == 0 is legal: zero totals, all-zero bucket_first / bucket_pos. The work is queued on hip_stream and the call
 * returns without waiting (the totals stay on the device); calls on one context are ordered through its steer scratch
 * (a buffer and an event of their own, as select's). Scratch: with g = ceil(n / 1024) blocks and K = n_buckets,
 * 12 * K * g + 12 * K + 8 * g bytes (per bucket and block a 32-bit count and a 64-bit byte sum, the K bucket totals,
 * two 32-bit counters per block); PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_steer_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_steer_spec* spec, pcppx_steering* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_steer_reference(const pcppx_batch* batch, const pcppx_steer_spec* spec, pcppx_steering* out);

/* ---- defrag: reassemble the IPv4 fragment groups that are complete inside one device batch (IPDefragUtil) ----
 * pcppx_reasm_device stops at the fragment table; this is the table's common case, for packets that sit in HBM:
 * what Examples/IPDefragUtil does with IPReassembly::processPacket (Packet++/src/IPReassembly.cpp:281-515). Fragment
 * groups that are complete and well formed inside the batch are reassembled on the device into an ordinary
 * pcppx_batch (parse it again: the datagram gets its L4 layer, hash5 and checksums); every other fragment is labelled
 * and left for the caller's host IPReassembly. Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * Inputs: a device batch, its records from a device parse (FIXED layout, max_layers >= 1, the same max_layers here; the
 * summary or, when it is NULL, the brief supplies n_layers; PACKED records are refused as in pcppx_reasm_device) and
 * info[n], the pcppx_reasm_info of the same batch. info is an input column: it is not recomputed, and any info is legal.
 *
 * Candidates: packet i is a candidate iff (info[i].ip_status & 15) == PCPPX_IPR_FRAGMENT, PCPPX_IPR_F_IPV6 is not set,
 * its descriptor is in bounds (the rule of select and steer: offsets[i] + caplens[i] <= data_len, the 64-bit wrap
 * checked) and its chain records an IPv4 layer: the first layer of protocol IPv4 among the first
 * min(n_layers, max_layers) entries, the one IPv4FragmentWrapper takes (IPReassembly.cpp:71-74). Then
 * ip_off = layer.offset, hdr = layer.hdr_len and len = layer.data_len - layer.hdr_len (getIPLayerPayloadSize(): a
 * trailer is excluded). The layer must lie inside the packet (hdr >= 20, hdr <= data_len, offset + data_len <= caplen:
 * always so for the records of a parse of this batch; records that say otherwise are never followed outside the
 * packet). A FRAGMENT packet without such a layer is not a candidate (it is LEFT).
 *
 * Groups: all candidates with the same ip_key. The 32-bit hash alone decides, exactly as m_FragmentMap is keyed by the
 * hash alone (IPReassembly.cpp:322-327). frag_offset and PCPPX_IPR_F_LAST are taken from info.
 *
 * Clean groups: sort a group by (frag_offset, source index). It is reassembled iff it has 2..PCPPX_DEFRAG_MAX_FRAGS
 * members, every len > 0, member k's frag_offset equals the sum of the len of the members before it (an exact tiling
 * from 0: no gap, overlap or duplicate), exactly the sorted-last member has PCPPX_IPR_F_LAST,
 * ip_off + hdr + total <= PCPPX_MAX_CAPLEN (ip_off / hdr: the first member's; total: the sum of the len) and
 * hdr + total <= 65535. For such a group the reference returns the same packet whatever order the members arrive in,
 * and returns it when the last one arrives: until the member at offset 0 arrives every other member has
 * frag_offset > currentOffset = 0 and is parked in the out-of-order list (processPacket :425-446); the member at
 * offset 0 allocates the packet from its own bytes (:355-376); from then on currentOffset is always the end of a
 * tiling prefix, so an arriving member either continues it (:394-423) or is parked, and matchOutOfOrderFragments
 * (:640-701) appends the parked members in offset order. Nothing is appended twice or dropped (no member is below
 * currentOffset, the duplicate path of :447-453), and gotLastFragment is raised exactly when the LAST member is
 * appended, which needs every member before it: on the arrival of the member with the highest source index. A group
 * that fails the rule is order-dependent or needs the host's duplicate handling: it stays with the host.
 *
 * The reassembled packet (IPReassembly.cpp:364-372, 409-415, 463-487; IPv4Layer.cpp:372-413): bytes
 * [0, ip_off + hdr + len) of the first member (its trailer dropped), then the payloads of the other members in offset
 * order; in the IP header at ip_off, bytes 2-3 = be16(hdr + total), bytes 6-7 = 0 (fragmentOffset = 0 clears DF too) and
 * bytes 10-11 = the header checksum over hdr bytes with the field zeroed. The protocol byte does not change:
 * computeCalculateFields rewrites it only to the value parseNextLayer dispatched on to build that next layer.
 *
 * Output, in source order: a reassembled packet takes the slot of its group's member with the highest source index
 * (where processPacket returns REASSEMBLED and IPDefragUtil writes it); the other members produce nothing. With
 * spec->passthrough = 1 every other in-bounds packet (non-fragments, HOST packets, IPv6 fragments, LEFT fragments) is
 * copied unchanged in place: IPDefragUtil's output file. With passthrough = 0 only the reassembled packets come out. */
#define PCPPX_DEFRAG_MAX_FRAGS 64
typedef struct pcppx_defrag_spec {
	uint32_t max_fragments; /* the candidates the call has room for; 0 = n (always enough) */
	uint8_t passthrough;    /* 0 / 1 */
	uint8_t reserved[3];
} pcppx_defrag_spec;

/* pcppx_defragged.disposition values */
#define PCPPX_DEFRAG_PASS 0        /* not an IPv4 fragment (in bounds) */
#define PCPPX_DEFRAG_LEFT 1        /* an IPv4 fragment of a group the device did not reassemble, or an IPv6 fragment,
                                      or a fragment of a family the spec does not ask for: the host table decides */
#define PCPPX_DEFRAG_MERGED 2      /* merged into a reassembled packet */
#define PCPPX_DEFRAG_MERGED_LAST 3 /* merged, and its output slot holds the packet */
#define PCPPX_DEFRAG_BAD_DESC 4    /* the descriptor is out of bounds: never read, never copied */

/* pcppx_defragged.totals words */
#define PCPPX_DEFRAG_OUT_PACKETS 0
#define PCPPX_DEFRAG_OUT_BYTES 1
#define PCPPX_DEFRAG_REASSEMBLED 2  /* clean groups = reassembled packets */
#define PCPPX_DEFRAG_MERGED_FRAGS 3 /* their members */
#define PCPPX_DEFRAG_LEFT_FRAGS 4   /* packets with disposition LEFT */
#define PCPPX_DEFRAG_CANDIDATES 5
#define PCPPX_DEFRAG_BAD_DESC_N 6   /* packets with disposition BAD_DESC */
#define PCPPX_DEFRAG_OVERFLOW 7
#define PCPPX_DEFRAG_TOTALS 8

typedef struct pcppx_defragged { /* all device pointers (host pointers for pcppx_defrag_reference) */
	uint8_t* data;        /* packed bytes of the output packets, back to back, no padding; NULL = index-only */
	uint64_t data_cap;
	uint64_t* offsets;    /* max_packets entries */
	uint32_t* caplens;    /* max_packets entries */
	uint32_t* index;      /* optional (NULL): index[j] = source packet number; a reassembled packet: the completing
	                         member's (strictly ascending) */
	uint32_t* first;      /* optional (NULL): the source number of the member whose headers, and so whose timestamp,
	                         packet j carries; a copied packet: index[j] */
	uint8_t* frags;       /* optional (NULL): members merged into packet j; 0 = a copied packet */
	uint8_t* disposition; /* optional (NULL): n entries, PCPPX_DEFRAG_* per source packet */
	uint32_t max_packets;
	uint32_t reserved;
	uint64_t* totals;     /* PCPPX_DEFRAG_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_defragged;

/* Capacity is all or nothing, as in steer: OVERFLOW = 1 iff OUT_PACKETS > max_packets, or data != NULL and
 * OUT_BYTES > data_cap, or CANDIDATES > max_fragments (0 = n). Then only the totals are written (no byte of data, no
 * entry of offsets / caplens / index / first / frags / disposition): they hold the full would-be values, except that
 * with CANDIDATES > max_fragments the groups cannot be formed and only CANDIDATES, BAD_DESC_N and OVERFLOW are given
 * (the other words are 0). max_packets = n, data_cap = the sum of the caplens and max_fragments = n always suffice: a
 * reassembled packet is no longer than its members together (the first member's prefix plus the other members'
 * payloads, each a part of its own packet). With data == NULL no bytes move, the byte capacity is not applied and
 * offsets hold the would-be positions.
 * As select and steer: a packet of any caplen is copied; the source may be gapped, unordered or overlapping;
 * out->data must not overlap batch->data. Source bytes are read only through aligned 16-B granules that hold a byte of
 * a packet that is emitted or merged. Nothing outside [0, OUT_BYTES) of data or past the first OUT_PACKETS entries of
 * the per-output columns is written. The output is a pure function of the inputs, bit-identical from run to run:
 * every output position comes from counts and scans; atomics only form sets and sums. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals, offsets or caplens; with n > 0 a
 * null info, records->layers, or records->summary and records->brief both; PACKED (or DENSE) records; max_layers 0 or
 * above PCPPX_MAX_LAYERS; passthrough above 1; a non-zero reserved field. The work is queued on hip_stream and the
 * call returns without waiting; calls on one context are ordered through its defrag scratch (a buffer and an event of
 * their own, as select's and steer's). Scratch: with g = ceil(n / 1024) blocks, F = min(max_fragments or n, n) and
 * C = the power of two >= max(2F, 64): 16 + 40 g + 40 F + 40 C bytes (block sums and bases, one record per candidate,
 * one group slot per table entry; the table is cleared by every call, so a max_fragments sized to the traffic saves
 * time as well as memory); PCPPX_E_NOMEM when it cannot be allocated.
 * The call is batch-local. A caller that keeps a host IPReassembly across batches must see that its table holds
 * nothing for a key before trusting a reassembled packet of that key (an earlier batch may have left fragments of it
 * there); the LEFT fragments are what it feeds that table. */
PCPPX_API int pcppx_defrag_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                  uint8_t max_layers, const pcppx_reasm_info* info, const pcppx_defrag_spec* spec,
                                  pcppx_defragged* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_defrag_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                     const pcppx_reasm_info* info, const pcppx_defrag_spec* spec, pcppx_defragged* out);

/* ---- defrag6: defrag for both families: the IPv6 fragment groups of a device batch are reassembled too ----
 * IPReassembly::processPacket keeps the fragments of IPv4 and IPv6 in one table and Examples/IPDefragUtil counts both;
 * pcppx_defrag_device leaves every IPv6 fragment to the host. This call takes the families the spec names. Everything
 * not said here is pcppx_defrag_device's contract: the inputs, pcppx_defragged, the dispositions and totals words, the
 * output order, passthrough, the all-or-nothing capacity rule, the 16-B granule rule, determinism, n == 0, the scratch
 * formula, the stream ordering (the two calls share one scratch buffer and event per context) and the batch-local
 * caveat. Added within ABI 7: new symbols only. With families = PCPPX_DEFRAG_FAM_V4 every output column and every
 * byte equals pcppx_defrag_device's (the same kernels run).
 *
 * Candidates. An IPv4 fragment (PCPPX_IPR_F_IPV6 not set) is a candidate by defrag's rule. With families other than
 * PCPPX_DEFRAG_FAM_V4 alone, packet i is an IPv6 candidate iff (info[i].ip_status & 15) == PCPPX_IPR_FRAGMENT,
 * PCPPX_IPR_F_IPV6 is set, its descriptor is in bounds and its chain records an IPv6 layer: the first layer of protocol
 * IPv6 among the first min(n_layers, max_layers) entries, the one IPv6FragmentWrapper takes (IPReassembly.cpp:147).
 * Then ip_off = layer.offset, hdr = layer.hdr_len (the fixed header and every extension parseExtensions walked:
 * hdr >= 48, one fragment header at least) and len = layer.data_len - hdr (getIPLayerPayloadSize()). The layer must lie
 * inside the packet (hdr <= data_len, offset + data_len <= caplen), as in defrag. len comes from the records, not from
 * the payload-length field: the reference's constructor clamps the layer to payloadLength + getHeaderLen()
 * (IPv6Layer.cpp:37-39), which counts the extension bytes twice, so up to hdr - 40 bytes of a trailer count as payload
 * there, and in the parse's data_len too. A group with such a member fails the tiling rule below and is LEFT, as it
 * must be: the reference takes its duplicate path.
 *
 * Families. With families = V4 an IPv6 fragment is LEFT and never enters a group: today's result. With families = V6
 * or V4 | V6 the candidates of both families form the groups, by ip_key alone as m_FragmentMap does
 * (IPReassembly.cpp:322-327), and CANDIDATES counts both. A group is clean only if all of its members are of one
 * family and the spec asks for that family: two families that collide in the 32-bit key are never appended to one
 * another, and with families = V6 an IPv4 candidate is LEFT and so is every IPv6 fragment it shares its key with (an
 * IPv4 FRAGMENT packet that is no candidate -- no IPv4 layer recorded -- joins no group under any spec).
 *
 * Clean groups: defrag's rule, word for word (2..PCPPX_DEFRAG_MAX_FRAGS members, every len > 0, an exact tiling from 0
 * by (frag_offset, source index), PCPPX_IPR_F_LAST on the sorted-last member only), with the same two bounds on the
 * first member's ip_off and hdr: ip_off + hdr + total <= PCPPX_MAX_CAPLEN (the intermediate packet of :364-372 and
 * :411 still holds the extensions) and hdr + total <= 65535 (the 16-bit store of :476). processPacket runs the same
 * lines for both families, so defrag's argument that the result does not depend on the order of arrival carries over.
 * One condition is added, on the first member of an IPv6 group: its extension chain, walked as parseExtensions does
 * (IPv6Layer.cpp:79-147) from the fixed header's next-header byte over [ip_off + 40, ip_off + hdr) -- types 0, 43 and
 * 60 are (len8 + 1) * 8 bytes long, type 44 is 8, type 51 is (len8 + 2) * 4 -- must end exactly at hdr, must hold a
 * fragment header (it need not be the last extension), and the last extension's next-header byte nh must not itself
 * be one of these five types: the parse of the longer, reassembled packet (:481) would walk on into the payload and
 * removeAllExtensions would cut more than hdr - 40 bytes. The walk takes at most (hdr - 40) / 8 steps and reads
 * nothing outside the packet. A chain that fails is one the records do not describe: the group is LEFT.
 *
 * The reassembled IPv6 packet (IPReassembly.cpp:472-496; IPv6Layer.cpp:179-187, 314-356), with T = total and
 * H = hdr: bytes [0, ip_off + 40) of the first member, then the payloads of all members in offset order from
 * ip_off + 40 on. removeAllExtensions cuts every extension of the first member, a Hop-by-Hop header ahead of the
 * fragment header too; the first member's trailer is dropped. Its length is ip_off + 40 + T. In the IPv6 header at
 * ip_off, byte 6 = nh and bytes 4-5 = be16(min(T, bswap16(T + H))): line 476 stores T + H without htobe16, the parse
 * of :481 clamps the layer to that byte-swapped value plus H (IPv6Layer.cpp:37-39), and computeCalculateFields writes
 * the clamped length minus the fixed header back. (T = 1488, H = 48: T + H = 0x0600, the field says 6 and the packet
 * is 1488 bytes behind its fixed header all the same; T = 1192: 1192.) A parse of the output sees what the
 * reference's caller sees. Nothing else changes: there is no checksum, and computeCalculateFields rewrites the
 * next-header byte only to the value parseNextLayer dispatched on. first / frags / index are as in defrag.
 *
 * PCPPX_E_INVAL before any device work: defrag's list, and families 0 or with a bit above PCPPX_DEFRAG_FAM_V6. */
#define PCPPX_DEFRAG_FAM_V4 1
#define PCPPX_DEFRAG_FAM_V6 2
typedef struct pcppx_defrag6_spec {
	uint32_t max_fragments; /* the candidates the call has room for; 0 = n (always enough) */
	uint8_t passthrough;    /* 0 / 1 */
	uint8_t families;       /* PCPPX_DEFRAG_FAM_* bits; 0 or bits above 3: PCPPX_E_INVAL */
	uint8_t reserved[2];    /* 0 */
} pcppx_defrag6_spec;
PCPPX_API int pcppx_defrag6_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                   uint8_t max_layers, const pcppx_reasm_info* info, const pcppx_defrag6_spec* spec,
                                   pcppx_defragged* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_defrag6_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                      const pcppx_reasm_info* info, const pcppx_defrag6_spec* spec,
                                      pcppx_defragged* out);

/* ---- tcpstream: reassemble the TCP connection sides that are clean inside one device batch (TcpReassembly) ----
 * pcppx_reasm_device stops at the connection table; this is the table's common case, for packets that sit in HBM:
 * what TcpReassembly::reassemblePacket (Packet++/src/TcpReassembly.cpp:81-486, line numbers below are that file's)
 * delivers to its OnMessageReady callback. Connection sides that are clean inside the batch are reassembled on the
 * device into contiguous stream bytes; every other packet is labelled and left for the caller's host TcpReassembly.
 * Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * Inputs: as defrag. A device batch, its FIXED records (max_layers >= 1, the same max_layers here; the summary or, when
 * it is NULL, the brief supplies hash5, n_layers and l4_layer; PACKED and DENSE records are refused) and info[n], an
 * input column that is never recomputed: any info and any hash5 are legal.
 *
 * Candidates: packet i is a candidate iff (info[i].tcp_status & 15) == PCPPX_TCPR_DATA, its descriptor is in bounds (the
 * shared rule, the 64-bit wrap checked), l4_layer < min(n_layers, max_layers) and that layer has protocol TCP (4), the
 * TCP header's first 20 bytes and the payload [offset + hdr_len, offset + hdr_len + info[i].tcp_payload) lie inside
 * caplen, and the chain records an IP layer: the first entry of protocol IPv4 (2) or IPv6 (3), which is
 * getLayerOfType<IPLayer>() (:96-100), whose source address (4 bytes at IP + 12, or 16 bytes at IP + 8) lies inside
 * caplen. From the bytes: seq = be32 at TCP + 4, the source port = the 2 raw bytes at TCP + 0 (:192), the source
 * address. SYN / FIN / RST come from info[i].tcp_status and len from info[i].tcp_payload. Records that point outside
 * the packet are never followed: such a packet is LEFT, as is every other DATA packet that is no candidate.
 *
 * Connections: all candidates with the same hash5; the 32-bit key alone decides, exactly as m_ConnectionList is keyed
 * (:141-147). Key 0 is legal. Side 0 is the (address family, address, port) of the connection's candidate with the
 * lowest source index, side 1 that of the lowest-index candidate that differs from side 0 (:195-225). A candidate that
 * matches neither is LEFT (:239-245: it returns before it touches any state) and affects nothing else.
 *
 * Clean sides: in source order, the side's first member fixes start = seq + (SYN ? 1 : 0) (:312-319), and
 * rel = (seq - start) mod 2^32. A side is reassembled iff
 *   1. no member has SYN and len > 0 (:409-410 would skip a sequence number);
 *   2. every data member (len > 0) has rel < 2^31, the side's total is < 2^31, and the data members sorted by rel tile
 *      [0, total) exactly: no gap, overlap or duplicate (a retransmission or a keep-alive leaves the side to the host);
 *   3. the side's lowest-index FIN-or-RST member has an index >= every data member of the side;
 *   4. the connection's lowest-index RST member (of either side) has an index >= every data member of both sides;
 *   5. with base_clear = 1: the side is in order (source order = rel order over its data members), or the other side
 *      has no data member besides, at most, its own first member;
 *   6. it has at least one data byte.
 * A side is judged on its own: one side of a connection may be clean and the other not.
 * For a clean side the callbacks deliver exactly each data member's whole payload, once, in rel order. `sequence`, the
 * side's next expected number, is start plus the length of a tiling prefix at all times: the first member sets it
 * (:317-319); a data member at `sequence` is delivered whole and advances it (:382-419), then checkOutOfOrderFragments
 * (:558-583) releases, whole and in rel order, the parked members that now continue the prefix; a member above
 * `sequence` is parked (:436-468, the list is unlimited with maxOutOfOrderFragments = 0); no member is ever below
 * `sequence` (the tiling has no overlap), so neither trimming path (:340-379, :586-627) runs. Zero-length members move
 * nothing (:385-400, :439-454; a zero-length SYN after the first is at most an ignored retransmission). What could
 * flush the parked list as "[N bytes missing]" or ignore later data is ruled out: the other-side flush (:297-305)
 * needs parked members of this side (not in order) while a data member of the other side arrives that is not that
 * side's first member (condition 5; with base_clear = 0 the flush does not exist); handleFinOrRst (:501-527) flushes
 * this side or closes the flow only on a FIN / RST of this side, which by condition 3 comes when every data member has
 * arrived and, the tiling being complete, none is parked, or on a RST (:258-261, :525-526), which by condition 4 comes
 * after all data of both sides; the flow is closed (:173-177) only by a RST or by the FIN of both sides, and this side
 * ignores data (:256-268) only after its own FIN / RST. When the last data member (by index) has arrived the prefix is
 * the whole tiling, so everything has been delivered.
 * Where this rule is stricter than the text of the issue that asked for it, the code of the reference decided: a
 * zero-length FIN / RST as a side's first member returns at :271-276 before `sequence` is set, and later data of that
 * side is ignored (:256), which condition 3 already says.
 *
 * Output: data holds the stream bytes of the clean sides back to back, ordered by the source index of each side's
 * first member; each stream is its data members' payloads in rel order. streams[j] describes stream j. The optional
 * per-packet columns give every source packet's part. */
typedef struct pcppx_tcpstream_spec {
	uint32_t max_segments; /* the candidates the call has room for; 0 = n (always enough) */
	uint8_t base_clear;    /* 0 / 1: TcpReassemblyConfiguration::enableBaseBufferClearCondition (the reference's default
	                          is 1). maxOutOfOrderFragments is modelled at its default 0 (unlimited) */
	uint8_t reserved[3];
} pcppx_tcpstream_spec;

/* pcppx_tcpstream_rec.flags */
#define PCPPX_TCPS_F_SYN 0x01 /* some member of the side has SYN */
#define PCPPX_TCPS_F_FIN 0x02
#define PCPPX_TCPS_F_RST 0x04
#define PCPPX_TCPS_F_OOO 0x08 /* the data members did not arrive in rel order */

typedef struct pcppx_tcpstream_rec { /* 32 bytes per clean side */
	uint64_t pos;      /* byte position of the stream in data */
	uint32_t bytes;    /* its length (< 2^31) */
	uint32_t flow_key; /* hash5 */
	uint32_t first;    /* source index of the side's first member */
	uint32_t segments; /* its data members */
	uint32_t peer;     /* the record number of the connection's other side, or 0xFFFFFFFF when that is not clean */
	uint8_t side;      /* 0 / 1 */
	uint8_t flags;     /* PCPPX_TCPS_F_* */
	uint8_t reserved[2];
} pcppx_tcpstream_rec;

/* pcppx_tcpstreams.disposition values */
#define PCPPX_TCPS_NOT_TCP 0  /* status other than DATA and HOST (in bounds) */
#define PCPPX_TCPS_HOST 1     /* status PCPPX_TCPR_HOST: the host decides, and it may belong to any connection */
#define PCPPX_TCPS_LEFT 2     /* a DATA packet the device did not reassemble: what the host TcpReassembly is fed */
#define PCPPX_TCPS_STREAM 3   /* a data member of a clean side: its payload is in data */
#define PCPPX_TCPS_CONTROL 4  /* a zero-length member (SYN / FIN / RST) of a clean side */
#define PCPPX_TCPS_BAD_DESC 5 /* the descriptor is out of bounds: never read */

/* pcppx_tcpstreams.totals words */
#define PCPPX_TCPS_STREAMS 0
#define PCPPX_TCPS_BYTES 1
#define PCPPX_TCPS_SEGMENTS 2   /* packets with disposition STREAM */
#define PCPPX_TCPS_LEFT_N 3     /* packets with disposition LEFT */
#define PCPPX_TCPS_CANDIDATES 4
#define PCPPX_TCPS_HOST_N 5     /* packets with disposition HOST */
#define PCPPX_TCPS_BAD_DESC_N 6 /* packets with disposition BAD_DESC */
#define PCPPX_TCPS_OVERFLOW 7
#define PCPPX_TCPS_TOTALS 8
#define PCPPX_TCPS_NONE 0xFFFFFFFFu

typedef struct pcppx_tcpstreams { /* all device pointers (host pointers for pcppx_tcpstream_reference) */
	uint8_t* data;                /* the stream bytes, back to back, no padding; NULL = index-only */
	uint64_t data_cap;
	pcppx_tcpstream_rec* streams; /* max_streams entries */
	uint8_t* disposition;         /* optional (NULL): n entries, PCPPX_TCPS_* per source packet */
	uint32_t* seg_stream;         /* optional (NULL): n entries, the record number of a STREAM / CONTROL packet's side,
	                                 else PCPPX_TCPS_NONE */
	uint32_t* seg_pos;            /* optional (NULL): n entries, a STREAM / CONTROL packet's rel (a STREAM packet's payload
	                                 is at streams[seg_stream].pos + seg_pos), else 0 */
	uint32_t max_streams;
	uint32_t reserved;
	uint64_t* totals;             /* PCPPX_TCPS_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_tcpstreams;

/* Capacity is all or nothing, as in steer and defrag: OVERFLOW = 1 iff STREAMS > max_streams, or data != NULL and
 * BYTES > data_cap, or CANDIDATES > max_segments (0 = n). Then only the totals are written (no byte of data, no entry
 * of streams or of the per-packet columns): they hold the full would-be values, except that with
 * CANDIDATES > max_segments the connections cannot be formed and only CANDIDATES, HOST_N, BAD_DESC_N and OVERFLOW are
 * given (the other words are 0), as in defrag. max_streams = n, data_cap = the sum of the caplens and max_segments = n
 * always suffice. With data == NULL no bytes move, the byte capacity is not applied and pos holds the would-be positions.
 * As the other movers: the source may be gapped, unordered or overlapping; out->data must not overlap batch->data. Source
 * bytes are read only through aligned 16-B granules that hold a byte of an emitted payload, or as single header bytes of
 * an in-bounds candidate. Nothing outside [0, BYTES) of data, past the first STREAMS entries of streams or the n entries
 * of the per-packet columns is written. The output is a pure function of the inputs, bit-identical from run to run:
 * positions come from counts, scans and rel; atomics only form sets, sums, minima and maxima. n == 0 is legal (zero
 * totals). PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals or streams; with n > 0 a
 * null info, records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS; base_clear above 1; a non-zero reserved field. The work is queued on hip_stream and the call returns
 * without waiting; calls on one context are ordered through its tcpstream scratch (a buffer and an event of their own).
 * Scratch: with g = ceil(n / 1024) blocks, F = min(max_segments or n, n) and C = the power of two >= max(2F, 64):
 * 16 + 40 g + 4 n + 64 F + 120 C bytes (block sums and bases, one word per packet, one record per candidate, one
 * connection slot with its two sides and one segment slot per table entry; the tables are cleared by every call);
 * PCPPX_E_NOMEM when it cannot be allocated.
 * The call is batch-local. A caller that keeps a host TcpReassembly across batches must know that its table holds
 * nothing for a key before trusting a stream of that key; the LEFT packets are what it feeds that table. HOST packets
 * may belong to any connection: with a non-zero HOST_N the result is conditional on what the host finds in them.
 * "[N bytes missing]" markers, retransmission trimming and timeouts stay with the host. */
PCPPX_API int pcppx_tcpstream_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                     uint8_t max_layers, const pcppx_reasm_info* info, const pcppx_tcpstream_spec* spec,
                                     pcppx_tcpstreams* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_tcpstream_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                        const pcppx_reasm_info* info, const pcppx_tcpstream_spec* spec,
                                        pcppx_tcpstreams* out);

/* ---- frag: split the IPv4 packets of a device batch into fragments (IPFragUtil) ----
 * The inverse of defrag, for packets that sit in HBM: what Examples/IPFragUtil does with
 * splitIPPacketToFragmentsBySize (Examples/IPFragUtil/main.cpp:153-238). Every chosen IPv4 packet whose IP payload is
 * larger than the fragment size is replaced, in place in the batch's order, by its fragments; the output is an ordinary
 * pcppx_batch (parse it, send it on, or hand it to pcppx_defrag_device, which gives the packets back). One source
 * packet produces up to 8,190 output packets. Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * Inputs: a device batch and its records from a device parse (FIXED layout, max_layers >= 1, the same max_layers here;
 * the summary or, when it is NULL, the brief supplies n_layers; PACKED and DENSE records are refused), as in defrag; no
 * pcppx_reasm_info is needed.
 *
 * The IPv4 layer of packet i: the first layer of protocol IPv4 among the first min(n_layers, max_layers) recorded
 * entries, the one getLayerOfType<IPv4Layer>() returns (main.cpp:168-172). ip_off = layer.offset, hdr = layer.hdr_len,
 * pay = layer.data_len - layer.hdr_len (getLayerPayloadSize(): a trailer behind the IP payload is excluded, a capture
 * cut short bounds it). The layer must lie inside the packet and describe a header: 20 <= hdr <= 60, hdr <= data_len,
 * offset + data_len <= caplen (always so for the records of a parse of this batch; records that say otherwise are
 * never followed outside the packet: the packet is NOT_V4). Every encapsulation the parse handles is covered, since
 * the layer comes from the records: VLAN, MPLS, SLL / SLL2, raw IP, GRE (the outer header) and so on.
 *
 * The fragment size fs of packet i: spec->frag_size (IPFragUtil's -s) in size mode; in mtu mode
 * fs = (mtu - hdr) & ~7 (>= 8, since mtu >= 68 and hdr <= 60).
 *
 * Disposition of source packet i, the first rule that applies:
 *   1 BAD_DESC    offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (the rule of select, steer and defrag):
 *                 never read, never emitted
 *   2 UNSELECTED  spec->keep != NULL and keep[i] == 0
 *   3 NOT_V4      no IPv4 layer as defined above is recorded (non-IP and IPv6 packets, chains that stopped early)
 *   4 ALREADY     be16(bytes 6-7 of the IP header) & 0x3FFF != 0: the packet is itself a fragment
 *   5 FITS        size mode: pay <= fs (main.cpp:175); mtu mode: hdr + pay <= mtu
 *   6 DF          spec->honor_df and bit 0x4000 of that word is set
 *   7 SPLIT       everything else (pay > fs in both modes: at least two fragments)
 * Two deliberate departures from the reference, which stay with the host: it re-fragments a packet that already is a
 * fragment with offsets restarting at 0 (which corrupts the datagram; here ALREADY packets are copied), and it
 * fragments IPv6 packets with a random fragment id (here IPv6 packets are NOT_V4). Without honor_df the reference's
 * behaviour holds: DF is ignored and cleared.
 *
 * Fragments of a SPLIT packet (main.cpp:105-119, 185-237; IPv4Layer.cpp:372-413): c = ceil(pay / fs) of them,
 * 2 <= c <= 8190. Fragment j (0 <= j < c) is bytes [0, ip_off + hdr) of the source followed by its payload bytes
 * [j * fs, min((j + 1) * fs, pay)), `piece` bytes; in its IP header, bytes 2-3 = be16(hdr + piece), bytes
 * 6-7 = be16((j * fs / 8) | (j < c - 1 ? 0x2000 : 0)) (all three flag bits of the source cleared, as the reference's
 * & 0xff1f does) and bytes 10-11 = the RFC 1071 header checksum over the hdr bytes with that field zeroed (an odd last
 * byte, which no real header has, padded with zero). Nothing else changes: the protocol byte stays, a trailer is
 * dropped. Its caplen is ip_off + hdr + piece.
 *
 * Output, in source order: a SPLIT packet's fragments take its place, in offset order. With spec->copy_rest = 1 every
 * other in-bounds packet (UNSELECTED, NOT_V4, ALREADY, FITS, DF) is copied unchanged in place: IPFragUtil with -a
 * (copyAllPacketsToOutputFile). With copy_rest = 0 only the fragments come out: IPFragUtil without -a. The caller's
 * -f / -d filters arrive as keep (pcppx_bpf_device's and pcppx_filter_device's matched[] are such columns). */
typedef struct pcppx_frag_spec {
	const uint8_t* keep; /* device, n bytes: packet i is considered iff keep[i] != 0. NULL = every packet */
	uint32_t frag_size;  /* size mode: a multiple of 8 in 8..65528. Exactly one of frag_size and mtu is non-zero */
	uint32_t mtu;        /* mtu mode: 68..65535 */
	uint8_t copy_rest;   /* 0 / 1 */
	uint8_t honor_df;    /* 0 / 1 */
	uint8_t reserved[6];
} pcppx_frag_spec;

/* pcppx_fragmented.disposition values */
#define PCPPX_FRAG_UNSELECTED 0
#define PCPPX_FRAG_NOT_V4 1
#define PCPPX_FRAG_ALREADY 2
#define PCPPX_FRAG_FITS 3
#define PCPPX_FRAG_DF 4
#define PCPPX_FRAG_SPLIT 5
#define PCPPX_FRAG_BAD_DESC 6

/* pcppx_fragmented.totals words */
#define PCPPX_FRAG_OUT_PACKETS 0   /* FRAGMENTS + COPIED */
#define PCPPX_FRAG_OUT_BYTES 1
#define PCPPX_FRAG_SPLIT_PACKETS 2 /* packets with disposition SPLIT */
#define PCPPX_FRAG_FRAGMENTS 3     /* their fragments */
#define PCPPX_FRAG_COPIED 4        /* packets copied unchanged (0 with copy_rest = 0) */
#define PCPPX_FRAG_UNDER_SIZE 5    /* packets with disposition FITS (whatever copy_rest) */
#define PCPPX_FRAG_BAD_DESC_N 6    /* packets with disposition BAD_DESC */
#define PCPPX_FRAG_OVERFLOW 7
#define PCPPX_FRAG_TOTALS 8

typedef struct pcppx_fragmented { /* all device pointers (host pointers for pcppx_frag_reference) */
	uint8_t* data;        /* packed bytes of the output packets, back to back, no padding; NULL = index-only */
	uint64_t data_cap;
	uint64_t* offsets;    /* max_packets entries */
	uint32_t* caplens;    /* max_packets entries */
	uint32_t* index;      /* optional (NULL): index[r] = source packet number of output packet r (non-decreasing) */
	uint16_t* frag_no;    /* optional (NULL): frag_no[r] = j for fragment j; 0 for a copied packet */
	uint16_t* counts;     /* optional (NULL): n entries: the output packets source packet i produced: 0, 1 or c */
	uint8_t* disposition; /* optional (NULL): n entries, PCPPX_FRAG_* per source packet */
	uint32_t max_packets;
	uint32_t reserved;
	uint64_t* totals;     /* PCPPX_FRAG_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_fragmented;

/* Capacity is all or nothing, as in steer and defrag: OVERFLOW = 1 iff OUT_PACKETS > max_packets, or data != NULL and
 * OUT_BYTES > data_cap. Then only the totals are written (no byte of data, no entry of offsets / caplens / index /
 * frag_no / counts / disposition), and they hold the full would-be values. Sizing: make an index-only call first
 * (data = NULL, max_packets = 0: it overflows and costs one pass over the records) and allocate OUT_PACKETS entries
 * and OUT_BYTES bytes; or use a closed bound. With head_i = ip_off_i + hdr_i, a SPLIT packet puts out
 * c_i * head_i + pay_i bytes, at most its caplen + (c_i - 1) * head_i, so
 *   OUT_BYTES <= sum caplen_i + sum (c_i - 1) * head_i   and   OUT_PACKETS <= n + sum (c_i - 1),
 * and from the descriptors alone, with F = frag_size (size mode) or (mtu - 60) & ~7 (mtu mode), c_i <= ceil(caplen_i / F),
 * head_i + pay_i <= caplen_i and so (c_i - 1) * head_i < pay_i * head_i / F <= caplen_i^2 / (4 F):
 *   OUT_PACKETS <= sum max(1, ceil(caplen_i / F))   and   OUT_BYTES <= sum (caplen_i + caplen_i^2 / (4 F)).
 * With data == NULL no bytes move, the byte capacity is not applied and offsets hold the would-be positions.
 * As the other movers: a packet of any caplen (0, or above PCPPX_MAX_CAPLEN) is copied; the source may be gapped,
 * unordered or overlapping; out->data must not overlap batch->data. Source bytes are read only through aligned 16-B
 * granules that hold a byte of a packet that is emitted, or as single bytes of the IPv4 header of an in-bounds,
 * selected packet. Nothing outside [0, OUT_BYTES) of data or past the first OUT_PACKETS entries of offsets / caplens /
 * index / frag_no is written, and nothing outside the n entries of counts / disposition. The output is a pure function
 * of the inputs, bit-identical from run to run: every position comes from counts and scans, and there are no atomics.
 * n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals, offsets or caplens; with n > 0 a
 * null records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS; frag_size and mtu both zero or both set; a frag_size that is not a multiple of 8 in 8..65528; an
 * mtu outside 68..65535; copy_rest or honor_df above 1; a non-zero reserved field. The work is queued on hip_stream
 * and the call returns without waiting; calls on one context are ordered through its frag scratch (a buffer and an
 * event of their own, as select's, steer's and defrag's). Scratch: with g = ceil(n / 1024) blocks, 52 g + 12 n bytes
 * (per block its output packets and bytes and their exclusive prefixes, 64-bit each, and five 32-bit counts; per
 * packet a 12-byte plan: the header's partial checksum, ip_off, pay, hdr and the disposition); PCPPX_E_NOMEM when it
 * cannot be allocated. */
PCPPX_API int pcppx_frag_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                uint8_t max_layers, const pcppx_frag_spec* spec, pcppx_fragmented* out,
                                void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_frag_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                   const pcppx_frag_spec* spec, pcppx_fragmented* out);

/* ---- frag6: frag for both families: the IPv6 packets of a device batch are split into fragments too ----
 * splitIPPacketToFragmentsBySize handles both families in one routine (Examples/IPFragUtil/main.cpp:153-238);
 * pcppx_frag_device labels every IPv6 packet NOT_V4 because the reference draws the IPv6 fragment id with rand(). Here
 * the ids are an input column, so the output stays a pure function of the inputs and that departure is closed: this
 * call takes the families the spec names. Everything not said here is pcppx_frag_device's contract: the inputs,
 * pcppx_fragmented, the totals words, the output order, keep and copy_rest, the all-or-nothing capacity rule, the
 * index-only sizing call, the 16-B granule rule, determinism (no atomics), n == 0, the scratch formula (52 g + 12 n
 * bytes: the plan's words are shared by the two families) and the stream ordering (the two calls share one scratch
 * buffer and event per context). Added within ABI 7: new symbols only. With families = PCPPX_FRAG_FAM_V4 every
 * output column and every byte equals pcppx_frag_device's (the same kernels run) and ids / id_base are ignored.
 *
 * Which layer (main.cpp:159-172: IPv4 if the packet has any IPv4 layer, else the first IPv6 layer). With V4 | V6: the
 * first recorded IPv4 layer if there is one, by frag's rule and with frag's dispositions (a 6in4 packet is split at
 * its IPv4 header, a 4in6 packet at its inner IPv4 header); otherwise the first layer of protocol IPv6 among the first
 * min(n_layers, max_layers) entries. With V6: a packet that records an IPv4 layer is NOT_IP (its datagram is the IPv4
 * one, and that family was not asked for); otherwise its first IPv6 layer is taken.
 *
 * The IPv6 candidate: ip_off = layer.offset, hdr = layer.hdr_len (the fixed header and every extension
 * parseExtensions walked, Packet++/src/IPv6Layer.cpp:79-147) and pay = layer.data_len - hdr (getLayerPayloadSize():
 * the records' value, with the constructor's clamp to payloadLength + getHeaderLen() already in it,
 * IPv6Layer.cpp:37-39). Required: 40 <= hdr <= data_len and offset + data_len <= caplen; otherwise the packet is
 * NOT_IP and nothing is read. Then the extension chain is walked from the next-header byte at ip_off + 6 over
 * [ip_off + 40, ip_off + hdr): types 0, 43 and 60 are (len8 + 1) * 8 bytes long, type 44 is 8, type 51 is
 * (len8 + 2) * 4. It yields nh_at, the packet offset of the last extension's next-header byte (ip_off + 6 without
 * extensions), and whether a type-44 header is among them. A chain that does not end exactly at hdr (a next header
 * that is no extension type ahead of hdr, an extension that crosses hdr) is one the records do not describe: NOT_IP.
 * The walk takes at most PCPPX_FRAG6_MAX_EXT steps and reads nothing outside [ip_off, ip_off + hdr).
 *
 * Disposition of an IPv6 candidate, after BAD_DESC, UNSELECTED and NOT_IP, the first rule that applies:
 *   1 LEFT     the chain is sound so far but has more than PCPPX_FRAG6_MAX_EXT extensions, or the chain is sound and
 *              a layer ahead of the IPv6 layer is not Ethernet, VLAN or SLL: the host's
 *   2 ALREADY  the chain holds a fragment header (the reference would add a second one and restart the offsets at 0:
 *              the same deliberate departure as for IPv4)
 *   3 FITS     size mode: pay <= fs; mtu mode: hdr + pay <= mtu
 *   4 LEFT     mtu mode only: mtu < hdr + 16 (no room for 8 payload bytes behind the fragment header)
 *   5 SPLIT    with fs = frag_size, or in mtu mode (mtu - hdr - 8) & ~7
 * honor_df has no meaning for IPv6 and is ignored there. LEFT packets are copied under copy_rest, as every other
 * unsplit packet.
 *
 * Fragments of a SPLIT IPv6 packet (main.cpp:124-128, 185-237; IPv6Layer.h:212-241; IPv6Extensions.cpp:52-69;
 * IPv6Layer.cpp:314-356): c = ceil(pay / fs) of them, 2 <= c <= 8187. Fragment j is bytes [0, ip_off + hdr) of the
 * source, then an 8-byte fragment header -- byte 0 the value the byte at nh_at held, byte 1 zero, bytes 2-3
 * be16((j * fs) | (j < c - 1 ? 1 : 0)), bytes 4-7 be32(id) -- then its payload bytes [j * fs, min((j + 1) * fs, pay)),
 * `piece` bytes. In the copied part the byte at nh_at becomes 44 and bytes ip_off + 4..5 become
 * be16(hdr - 40 + 8 + piece). Nothing else changes from ip_off on: there is no checksum, a trailer is dropped. Its caplen is
 * ip_off + hdr + 8 + piece, which can exceed the source's caplen by up to 7 bytes (the movers emit any caplen). The
 * fragment id of source packet i is ids ? ids[i] : (uint32_t)(id_base + i), wrapping at 2^32.
 *
 * The layers ahead of the IPv6 header. Packet::computeCalculateFields runs over every layer of a fragment, and the
 * layers in front recompute fields of their own: a PPPoE or GRE v1 length, a tunnel's UDP length and checksum, and so
 * on, per fragment. So an IPv6 candidate is split only if every layer recorded ahead of its IPv6 layer is Ethernet,
 * VLAN or SLL (none at all: raw IP); any other layer there makes it LEFT (rule 1 below), decided from the records
 * alone. Of those three, each sets its type field from the layer behind it (EthLayer.cpp:71-93, VlanLayer.cpp:121-143,
 * SllLayer.cpp:104-126), which changes a byte in one case only: ahead of a VLAN layer the field becomes 0x8100, so an
 * 802.1ad tag's 0x88A8 is renamed. Every fragment carries that: for each layer k ahead of the IPv6 layer whose
 * successor k + 1 is a VLAN layer with 2 <= offset <= ip_off, bytes offset - 2 and offset - 1 are 0x81 0x00 (written,
 * never read). tests/golden/frag6 records it behind Ethernet, VLAN and SLL. (pcppx_frag_device copies those bytes.)
 *
 * Sizes: a SPLIT IPv6 packet puts out c * (ip_off + hdr + 8) + pay bytes, so frag's closed bound gains 8 * c_i:
 *   OUT_BYTES <= sum caplen_i + sum (c_i - 1) * head_i + 8 * sum c_i,
 * and from the descriptors alone, with F = frag_size in size mode and in mtu mode
 * F = min((mtu - 60) & ~7, (mtu - H - 8) & ~7), H = min(the largest IPv6 hdr in the batch, mtu - 16) (a packet with
 * hdr > mtu - 16 is never split; H = mtu - 16 always holds and gives F = 8),
 *   OUT_PACKETS <= sum max(1, ceil(caplen_i / F))   and
 *   OUT_BYTES <= sum (caplen_i + caplen_i^2 / (4 F) + 8 * ceil(caplen_i / F)).
 * Source bytes are read as in frag, and as single bytes of the IPv6 header and extensions of an in-bounds, selected
 * packet. An IPv6 fragment's bytes differ from the source's only in the places named above.
 *
 * PCPPX_E_INVAL before any device work: frag's list, and families 0 or with a bit above PCPPX_FRAG_FAM_V6. */
#define PCPPX_FRAG_FAM_V4 1
#define PCPPX_FRAG_FAM_V6 2
#define PCPPX_FRAG6_MAX_EXT 16
/* two more pcppx_fragmented.disposition values */
#define PCPPX_FRAG_NOT_IP PCPPX_FRAG_NOT_V4 /* no layer of a family the spec asks for, as defined above */
#define PCPPX_FRAG_LEFT 7                   /* an IPv6 packet this call does not split and the reference would */
typedef struct pcppx_frag6_spec {
	const uint8_t* keep; /* as pcppx_frag_spec */
	uint32_t frag_size;
	uint32_t mtu;
	uint8_t copy_rest;
	uint8_t honor_df;    /* IPv4 packets only */
	uint8_t families;    /* PCPPX_FRAG_FAM_* bits; 0 or bits above 3: PCPPX_E_INVAL */
	uint8_t reserved[5]; /* 0 */
	const uint32_t* ids; /* device, n entries: the fragment id of source packet i. NULL: (uint32_t)(id_base + i) */
	uint32_t id_base;
	uint32_t reserved2;  /* 0 */
} pcppx_frag6_spec;
PCPPX_API int pcppx_frag6_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                 uint8_t max_layers, const pcppx_frag6_spec* spec, pcppx_fragmented* out,
                                 void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_frag6_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                    const pcppx_frag6_spec* spec, pcppx_fragmented* out);

/* ---- tlsfp: JA3 / JA3S TLS fingerprints of the hello packets of a device batch (TLSFingerprinting) ----
 * What Examples/TLSFingerprinting does with SSLClientHelloMessage::generateTLSFingerprint() and
 * SSLServerHelloMessage::generateTLSFingerprint() and their toStringAndMD5() (Packet++/src/SSLHandshake.cpp:1577-1689,
 * 1892-1950; Examples/TLSFingerprinting/main.cpp:328-381), for packets that sit in HBM: per ClientHello / ServerHello
 * packet one record with the fingerprint text's MD5, the text itself and the packet's number (which indexes
 * pcppx_tuple for the addresses and ports of the example's output file; md5's first word is a 32-bit key for
 * pcppx_steer_device or pcppx_flow_count_keys_device). Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * Inputs: as frag. A device batch and its FIXED records (max_layers >= 1, the same value as the parse used; the summary
 * or, when it is NULL, the brief supplies flags and n_layers; PACKED and DENSE records are refused). No
 * pcppx_reasm_info is needed.
 *
 * Per packet i the first rule that applies decides (be16(x): the big-endian 16-bit word at byte x):
 *   1 BAD_DESC. offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (the rule of select, steer, defrag and
 *     frag): the packet is never read.
 *   2 The handshake layer: the first entry k < min(n_layers, max_layers) with proto == 18 (pcpp::SSL) that lies inside
 *     the packet (data_len >= 5, hdr_len >= 5, hdr_len <= data_len, offset + data_len <= caplen) and whose byte at
 *     `offset` is 22: getLayerOfType<SSLHandshakeLayer>() (SSLLayer.cpp:42-56, main.cpp:335). An entry that points
 *     outside the packet is never followed. R = hdr_len - 5 is the record's data length as the constructor clamps it
 *     (SSLLayer.cpp:126-136). Only this layer is looked at: a hello in a later handshake record is not found, as in the
 *     reference.
 *   3 No handshake layer: HOST when the chain may hold one the device did not record -- flags has
 *     PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC or DEPTH_OVERFLOW, or n_layers > max_layers, or NEEDS_HOST_L7 is set
 *     with L7_SSL set or without L7_KNOWN. Otherwise NONE (a parse-until option that cut the chain short is the caller's
 *     choice).
 *   4 Messages (SSLLayer.cpp:138-149, SSLHandshake.cpp:1287-1350, 2257-2262): cur = 0; loop: D = R - cur, stop when
 *     D < 4; the message starts at offset + 5 + cur; it is unknown, takes all of D and ends the walk when D >= 16 and
 *     either its first five bytes are zero or its byte 1 is >= 1; otherwise its type is byte 0 and its length
 *     M = min(4 + be16(2), D); cur += M. With spec->client the first message of type 1 makes the packet CLIENT;
 *     otherwise, with spec->server, the first message of type 2 makes it SERVER (ClientHello wins when a record holds
 *     both, main.cpp:339-377); otherwise NONE. Below, byte positions count from the message's first byte, and the
 *     bound of every field read is D, the rest of the record, not M; only the extension list is cut at M.
 *   5 Shared pieces. Session id: sid = D <= 39 ? 0 : min(byte 38, D - 39). Extension list at E
 *     (SSLHandshake.cpp:1366-1449, 1695-1773, SSLHandshake.h:151-165): none when E + 2 > D; otherwise it = E + 2,
 *     end = min(it + be16(E), M), and while end - it >= 4 (as signed numbers): type = be16(it), len = be16(it + 2); stop
 *     when end - it < 4 + len; append (type, data at it + 4, len); it += 4 + len. GREASE: a 16-bit value whose two
 *     bytes are equal with low nibble 0xA (the set at SSLHandshake.cpp:1040-1053).
 *   6 ClientHello text (SSLHandshake.cpp:1451-1527, 1577-1677): "version,ciphers,extensions,groups,formats", every
 *     number unsigned decimal without padding, lists joined by '-', empty lists empty. version = D < 6 ? 0 : be16(4).
 *     cs = 39 + sid, count = cs + 2 > D ? 0 : be16(cs) / 2; cipher entry i < count is used while
 *     cs + 2 + 2 (i + 1) <= D, GREASE removed. E = cs + 2 + 2 count + 2: the reference assumes exactly one compression
 *     method and uses count, not the number of valid entries; both quirks are kept. Extensions: the types, GREASE
 *     removed. Groups: of the first listed extension of type 10, used only when len >= 2, be16(data) == len - 2 and that
 *     value is even; GREASE removed. Formats: of the first listed extension of type 11, used only when len >= 1 and
 *     len == data[0] + 1; one decimal per byte. Both are searched in the unfiltered list.
 *   7 ServerHello text (SSLHandshake.cpp:1775-1940): "version,cipher,extensions". cipher = 39 + sid + 2 > D ? 0 :
 *     be16(39 + sid); E = 39 + sid + 3; the extension types are not GREASE-filtered. version: of the first listed
 *     extension of type 43, len == 2 gives be16(data), len == 3 with data[0] == 2 gives be16(data + 1); otherwise
 *     D < 6 ? 0 : be16(4). One deliberate departure: with that extension at len == 0 the reference dereferences a null
 *     getData(); here the header's version is used.
 *   8 md5 is the RFC 1321 digest of the text's bytes. */
typedef struct pcppx_tlsfp_spec {
	uint32_t max_hellos; /* the hello packets the call has room for; 0 = n (always enough) */
	uint8_t client;      /* 0 / 1: ClientHello fingerprints (the example's -t ch) */
	uint8_t server;      /* 0 / 1: ServerHello fingerprints (-t sh); both = ch_sh; at least one */
	uint8_t reserved[2];
} pcppx_tlsfp_spec;

#define PCPPX_TLSFP_CLIENT 1 /* pcppx_tlsfp_rec.kind (and the disposition of its packet) */
#define PCPPX_TLSFP_SERVER 2
typedef struct pcppx_tlsfp_rec { /* 40 bytes per fingerprint */
	uint8_t md5[16];     /* RFC 1321 digest of the text; md5[0] is the first byte of toMD5()'s hex string */
	uint64_t text_pos;   /* byte position of the text in out->text */
	uint32_t text_len;
	uint32_t index;      /* source packet number (strictly ascending) */
	uint16_t msg_offset; /* the hello message's first byte, from the packet's first byte (its low 16 bits, where
	                        crafted records place the layer past byte 65,535 of an oversize packet) */
	uint8_t kind;        /* PCPPX_TLSFP_CLIENT / PCPPX_TLSFP_SERVER */
	uint8_t reserved[5]; /* written as 0 */
} pcppx_tlsfp_rec;

/* pcppx_tlsfps.disposition values */
#define PCPPX_TLSFP_NONE 0     /* no hello the spec asks for (in bounds) */
/*      PCPPX_TLSFP_CLIENT 1      a record of kind CLIENT */
/*      PCPPX_TLSFP_SERVER 2      a record of kind SERVER */
#define PCPPX_TLSFP_HOST 3     /* no recorded handshake layer, but the host's chain may hold one (rule 3) */
#define PCPPX_TLSFP_BAD_DESC 4 /* the descriptor is out of bounds: never read */

/* pcppx_tlsfps.totals words */
#define PCPPX_TLSFP_CLIENT_N 0
#define PCPPX_TLSFP_SERVER_N 1
#define PCPPX_TLSFP_TEXT_BYTES 2
#define PCPPX_TLSFP_HOST_N 3
#define PCPPX_TLSFP_BAD_DESC_N 4
#define PCPPX_TLSFP_CANDIDATES 5 /* hello packets: CLIENT_N + SERVER_N */
/* word 6 is zero */
#define PCPPX_TLSFP_OVERFLOW 7
#define PCPPX_TLSFP_TOTALS 8

typedef struct pcppx_tlsfps {  /* device pointers; host pointers for pcppx_tlsfp_reference */
	pcppx_tlsfp_rec* recs;     /* max_recs entries, in source order */
	uint8_t* text;             /* the fingerprint texts back to back in record order, no terminator; NULL = MD5 only */
	uint64_t text_cap;
	uint8_t* disposition;      /* optional (NULL): n entries, PCPPX_TLSFP_* per source packet */
	uint32_t max_recs;
	uint32_t reserved;
	uint64_t* totals;          /* PCPPX_TLSFP_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_tlsfps;

/* Capacity is all or nothing, as in frag and defrag: OVERFLOW = 1 iff CLIENT_N + SERVER_N > max_recs, or text != NULL
 * and TEXT_BYTES > text_cap, or CANDIDATES > max_hellos (0 = n). Then only the totals are written (no record, no byte
 * of text, no disposition): they hold the full would-be values, except that with CANDIDATES > max_hellos only
 * CANDIDATES, HOST_N, BAD_DESC_N and OVERFLOW are given (the other words are 0). With text == NULL the digests are
 * still computed, text_pos holds the would-be positions and the byte capacity is not applied. Sizing: a call with
 * max_recs = 0 overflows and gives CLIENT_N + SERVER_N and TEXT_BYTES; or use the closed bound
 * text_len <= 4 * caplen + 16 (a point-format byte prints as at most 4 characters, two list bytes as at most 6).
 * One packet may hold ~32k cipher entries and make one lane walk ~190 KB of text while its wave waits: the cost of a
 * hello is bounded by PCPPX_MAX_CAPLEN bytes of it, as in the reference.
 * Source bytes are read only from in-bounds packets, inside a recorded SSL layer that lies inside the packet. Nothing
 * is written outside the first CLIENT_N + SERVER_N records, [0, TEXT_BYTES) of the text and the n dispositions. The
 * output is a pure function of the inputs, bit-identical from run to run: positions come from counts and scans, and
 * there are no atomics. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals or recs; with n > 0 a null
 * records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS; client and server both 0, or either above 1; a non-zero reserved field. The work is queued on
 * hip_stream and the call returns without waiting; calls on one context are ordered through its tlsfp scratch (a buffer
 * and an event of their own, as frag's). Scratch: with g = ceil(n / 1024) blocks, 48 g + 16 n bytes (per block its
 * records and text bytes and their exclusive prefixes, 64-bit each, and four 32-bit counts; per packet a 16-byte plan:
 * the message's offset, D, M, the text's length and the disposition); PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_tlsfp_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                 uint8_t max_layers, const pcppx_tlsfp_spec* spec, pcppx_tlsfps* out,
                                 void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_tlsfp_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                    const pcppx_tlsfp_spec* spec, pcppx_tlsfps* out);

/* ---- dns: DnsLayer's resource records of the DNS packets of a device batch ----
 * What DnsLayer::parseResources and IDnsResource::decodeName do (Packet++/src/DnsLayer.cpp:133-220,
 * DnsResource.cpp:33-155), for packets that sit in HBM: per DNS packet one message record, per linked query / answer /
 * authority / additional resource one record with its decoded name. It is what the dns mode of
 * Examples/PcapPlusPlus-benchmark/benchmark.cpp:30-52 walks. Added within ABI 7: new symbols only (PCPPX_ABI_VERSION
 * stays 7).
 *
 * Inputs: as tlsfp. A device batch and its FIXED records (max_layers >= 1, the same value as the parse used; the summary
 * or, when it is NULL, the brief supplies flags and n_layers; PACKED and DENSE records are refused).
 *
 * Per packet i the first rule that applies decides (be16(x): the big-endian 16-bit word at byte x):
 *   1 BAD_DESC. offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (the rule of select, steer, defrag, frag and
 *     tlsfp): the packet is never read.
 *   2 The DNS layer: the first entry k < min(n_layers, max_layers) with proto == 13 (pcpp::DNS):
 *     getLayerOfType<DnsLayer>(). L = data_len (m_DataLen). adj = 2 when k >= 1 and entry k - 1 has proto == 4 (TCP):
 *     DnsOverTcpLayer (DnsLayer.h:439-441, TcpLayer.cpp:411-415), otherwise 0. The entry is followed only when it lies
 *     inside the packet (hdr_len <= data_len and offset + data_len <= caplen) and L >= 12 + adj; otherwise the packet is
 *     NONE and no later entry is looked at (a parse of this batch never writes such an entry).
 *   3 No entry with proto == 13: HOST when the host's chain may hold a DNS layer the device did not record -- flags has
 *     PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC or DEPTH_OVERFLOW, or n_layers > max_layers, or NEEDS_HOST_L7 is set
 *     with L7_DNS set or without L7_KNOWN. Otherwise NONE.
 *   4 The message (DnsLayer.cpp:133-220); positions count from the layer's first byte. id = be16(adj), flags =
 *     be16(adj + 2); the four declared counts are be16 at adj + 4, 6, 8 and 10. If their sum is above 300 no resource is
 *     linked: status TOO_MANY. Otherwise off = 12 + adj and, for each of sum resources: its section is the first of
 *     query, answer, authority, additional whose count is still non-zero (which is then decremented); name_len and the
 *     text come from rule 5 at off; a query has size = name_len + 4; any other resource has size = name_len + 10 + dl
 *     with dl = 0 when off + name_len + 8 >= L - 1 (DnsResource.cpp:281-295), else be16(off + name_len + 8). If
 *     off + size > L the walk stops with status TRUNCATED, and that resource and all after it are not linked; otherwise
 *     the resource is linked and off += size. type, class, TTL and dl of a linked resource are read at off + name_len
 *     (in bounds by the size check). A name whose decode fails has name_len 0 and an empty name; its resource is still
 *     linked when its 4 / 10 bytes fit, as in the reference.
 *   5 decodeName (DnsResource.cpp:33-155) at position off, level 1 (its `iteration` argument starts at 1,
 *     DnsResource.h:43), with all its quirks. A level is empty (name_len 0, no failure) when off + 1 > L or level > 20:
 *     a name is its own labels and at most 19 pointers deep. Otherwise enc = 0, cur = off, and while byte w at cur is not 0:
 *       a pointer (w & 0xC0 == 0xC0): if cur + 2 > L or enc > 255 the level ends as with a zero byte. Otherwise
 *         to = ((w & 0x3F) << 8 | byte(cur + 1)) + adj, modulo 2^16; to < 12 or to >= L makes the level fail (name_len 0;
 *         the text it gathered so far stays, which matters for a nested level); otherwise the level below (at `to`,
 *         level + 1) is decoded, its text is cut at its first NUL byte, and as much of it as leaves this level's text at
 *         255 bytes or less is appended; name_len = enc + 2, and no trailing dot is removed.
 *       a label (every other w, 0x40-0xBF included): if cur + w + 1 > L or enc + w > 255 the level ends cut: with
 *         enc == 256 its last text byte is dropped and name_len = 256, else name_len = enc + 1 and the text keeps its
 *         trailing dot. Otherwise the label's w bytes and a '.' join the text, cur and enc grow by w + 1, and if then
 *         cur + 1 > L the level ends cut in the same way.
 *     At the zero byte (cleanup()): the text loses its last byte (the dot) when it has one, and name_len = enc + 1, or
 *     enc when the text had 256 bytes. Every level counts its own enc. The resource's name is empty when level 1 failed
 *     or name_len is 0; otherwise it is the text up to its first NUL byte (std::string from a C string): at most 255
 *     bytes (text_len <= 511 is a safe bound). The implementation has no recursion: after a pointer a level only
 *     returns, so a name is a chain of at most 20 label runs under one running byte budget. */
typedef struct pcppx_dns_spec {
	uint32_t max_msgs;   /* the DNS packets the call has room for; 0 = n (always enough) */
	uint8_t sections;    /* bits 0-3: resource records of queries, answers, authorities, additionals; non-zero */
	uint8_t reserved[3];
} pcppx_dns_spec;

#define PCPPX_DNS_QUERY 0 /* pcppx_dns_rr.section, and the index into declared[] / linked[] */
#define PCPPX_DNS_ANSWER 1
#define PCPPX_DNS_AUTHORITY 2
#define PCPPX_DNS_ADDITIONAL 3

/* pcppx_dns_msg.status */
#define PCPPX_DNS_COMPLETE 0  /* every declared resource is linked */
#define PCPPX_DNS_TRUNCATED 1 /* a resource reached past the layer's end: it and all after it are not linked */
#define PCPPX_DNS_TOO_MANY 2  /* more than 300 declared resources: none is linked */

typedef struct pcppx_dns_msg { /* 40 bytes per DNS packet */
	uint64_t first_rr;     /* record number in out->rrs of its first resource record */
	uint32_t index;        /* source packet number (strictly ascending) */
	uint16_t layer_offset; /* the DNS layer's first byte, from the packet's first byte */
	uint16_t layer_len;    /* L */
	uint16_t id;           /* be16(adj): dnshdr.transactionID */
	uint16_t flags;        /* be16(adj + 2): the header's flag bits as one big-endian word */
	uint16_t declared[4];  /* the header's four counts */
	uint16_t linked[4];    /* the resources linked per section, whatever spec->sections says */
	uint16_t n_rr;         /* the resource records emitted for it: linked[] of the sections in spec->sections */
	uint8_t adjust;        /* adj: 2 for DNS over TCP, else 0 */
	uint8_t status;        /* PCPPX_DNS_COMPLETE / TRUNCATED / TOO_MANY */
} pcppx_dns_msg;

typedef struct pcppx_dns_rr { /* 32 bytes per linked resource of a section in spec->sections, in walk order */
	uint64_t name_pos;    /* byte position of the decoded name in out->names */
	uint32_t msg;         /* its message's record number in out->msgs */
	uint32_t ttl;         /* DnsResource::getTTL(); 0 for a query */
	uint16_t offset;      /* m_OffsetInLayer: the resource's first byte, from the layer's first byte */
	uint16_t name_len;    /* m_NameLength: the encoded name's bytes as decodeName counts them */
	uint16_t text_len;    /* bytes of the decoded name (getName().size()) */
	uint16_t type;        /* getDnsType() */
	uint16_t dns_class;   /* getDnsClass() */
	uint16_t data_len;    /* getDataLength(); 0 for a query */
	uint16_t data_offset; /* getDataOffset(): offset + name_len + 10; 0 for a query */
	uint8_t section;      /* PCPPX_DNS_QUERY .. PCPPX_DNS_ADDITIONAL */
	uint8_t reserved;     /* written as 0 */
} pcppx_dns_rr;

/* pcppx_dns_out.disposition values */
#define PCPPX_DNS_NONE 0     /* no DNS layer that is followed (in bounds) */
#define PCPPX_DNS_MSG 1      /* a message record */
#define PCPPX_DNS_HOST 2     /* no recorded DNS layer, but the host's chain may hold one (rule 3) */
#define PCPPX_DNS_BAD_DESC 3 /* the descriptor is out of bounds: never read */

/* pcppx_dns_out.totals words */
#define PCPPX_DNS_MSGS 0
#define PCPPX_DNS_RRS 1
#define PCPPX_DNS_NAME_BYTES 2
#define PCPPX_DNS_HOST_N 3
#define PCPPX_DNS_BAD_DESC_N 4
#define PCPPX_DNS_QA_LINKED 5 /* linked queries + answers of all messages, whatever spec->sections says: the number
                                 `benchmark <file> dns 1` prints */
/* word 6 is zero */
#define PCPPX_DNS_OVERFLOW 7
#define PCPPX_DNS_TOTALS 8

typedef struct pcppx_dns_out { /* device pointers; host pointers for pcppx_dns_reference */
	pcppx_dns_msg* msgs;       /* max_msgs entries, in source order */
	pcppx_dns_rr* rrs;         /* max_rrs entries: message by message, each in walk order */
	uint8_t* names;            /* the decoded names back to back in record order, no terminator; NULL = no text */
	uint64_t names_cap;
	uint8_t* disposition;      /* optional (NULL): n entries, PCPPX_DNS_* per source packet */
	uint32_t max_msgs;
	uint32_t max_rrs;
	uint64_t* totals;          /* PCPPX_DNS_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_dns_out;

/* Capacity is all or nothing, as in tlsfp: OVERFLOW = 1 iff MSGS > out->max_msgs, or RRS > max_rrs, or names != NULL
 * and NAME_BYTES > names_cap, or MSGS > spec->max_msgs (0 = n). Then only the totals are written (no record, no byte of
 * a name, no disposition); they always hold the full would-be values. With names == NULL positions and lengths are
 * still filled and the byte capacity is not applied. Sizing: a call with max_msgs = max_rrs = 0 overflows and gives
 * MSGS, RRS and NAME_BYTES. The cost of a packet is bounded: at most 300 resources, 20 label runs each, inside the
 * layer's L bytes.
 * Source bytes are read only from in-bounds packets, inside a recorded DNS layer that lies inside the packet. Nothing
 * is written outside the first MSGS messages, the first RRS records, [0, NAME_BYTES) of names and the n dispositions.
 * The output is a pure function of the inputs, bit-identical from run to run: positions come from counts and scans, and
 * there are no atomics. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals, msgs or rrs; with n > 0 a null
 * records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS; sections 0 or above 15; a non-zero reserved field. The work is queued on hip_stream and the call
 * returns without waiting; calls on one context are ordered through its dns scratch (a buffer and an event of their
 * own, as tlsfp's). Scratch: with g = ceil(n / 1024) blocks, 48 g + 16 n bytes (per block six 32-bit sums -- its
 * messages, records, name bytes, HOST and BAD_DESC packets, queries plus answers -- and the 64-bit exclusive prefixes
 * of the first three; per packet a 16-byte plan: the layer's offset, length and adjustment, the records and name bytes
 * of the message, its queries plus answers, and the disposition);
 * PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_dns_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                               uint8_t max_layers, const pcppx_dns_spec* spec, pcppx_dns_out* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_dns_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                  const pcppx_dns_spec* spec, pcppx_dns_out* out);

/* ---- http: the first line and the header fields of the HTTP packets of a device batch ----
 * What HttpRequestFirstLine / HttpResponseFirstLine and TextBasedProtocolMessage::parseFields build
 * (Packet++/src/HttpLayer.cpp:166-320, :850-985, TextBasedProtocol.cpp:87-139, :448-541), for packets that sit in HBM:
 * per HTTP packet one message record (method, URI or status, version, header length, field count, content length),
 * per header field the caller asked for one record, and the bytes it asked for back to back. It is what
 * Examples/HttpAnalyzer reads of a packet (the method, the URI, getFieldByName("Host"), the status code,
 * Content-Length, Content-Type, the header size). Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * Inputs: as dns. A device batch and its FIXED records (max_layers >= 1, the same value as the parse used; the summary
 * or, when it is NULL, the brief supplies flags and n_layers; PACKED and DENSE records are refused).
 *
 * Per packet i the first rule that applies decides. Positions count from the layer's first byte; d[x] is the byte
 * at x:
 *   1 BAD_DESC. offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (the rule of select, steer, defrag, frag,
 *     tlsfp and dns): the packet is never read.
 *   2 The HTTP layer: the first entry k < min(n_layers, max_layers) with proto == 6 (pcpp::HTTPRequest) or 7
 *     (HTTPResponse). It is followed only when it lies inside the packet (hdr_len <= data_len and offset + data_len <=
 *     caplen); otherwise the packet is NONE and no later entry is looked at. L = data_len (m_DataLen), kind =
 *     proto - 6. A kind that is not in spec->kinds makes the packet NONE.
 *   3 No such entry: HOST when the host's chain may hold an HTTP layer the device did not record -- flags has
 *     PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC or DEPTH_OVERFLOW, or n_layers > max_layers, or NEEDS_HOST_L7 is set
 *     with L7_HTTP set or without L7_KNOWN. Otherwise NONE.
 *   4 A request's first line (HttpLayer.cpp:166-213, parseMethod :261-285, parseVersion :287-320, getUri :361-370).
 *     The method is the text before the first space, looked up among GET HEAD POST PUT DELETE TRACE OPTIONS CONNECT
 *     PATCH; it needs L >= 4 and the space at 1..L-1, and is 9 (unknown) otherwise. An unknown method gives
 *     first_line_len = L, version 3, no URI, not complete. Otherwise u = len(method) + 1 and v is the first " HTTP/"
 *     in [u, L). With no v, or v + 9 > L: version 3, no URI, first_line_len = L, not complete. Otherwise the version
 *     comes from d[v+6..v+8] ("0.9", "1.0", "1.1", else 3) and the URI is [u, v); with e the first '\n' in [v + 6, L)
 *     the line is complete with first_line_len = e + 1, and with no e it is L and not complete.
 *   5 A response's first line (parseStatusCode :850-895, the constructor :897-929, parseVersion :964-985). The version
 *     is known when L >= 8, the layer starts with "HTTP/" and d[5..7] is one of the three texts. status_code is the
 *     number in d[9..11] when the version is known, L >= 12, the three bytes are digits, a '\n' exists in [13, L) and
 *     the bytes between 13 and that '\n', less one trailing '\r', are not empty: those bytes are the status message.
 *     Otherwise status_code is 0 and there is no message. No code table is consulted: a layer the parse recorded
 *     always has a supported code. first_line_len is one past the first '\n' in [0, L), else L; complete means that
 *     '\n' exists.
 *   6 A field at off (HeaderField, TextBasedProtocol.cpp:448-541), e the first '\n' in [off, L): size = e - off + 1;
 *     with no e, size is the bytes up to the first NUL or to L (:455-461). It is an end-of-header field when size == 0
 *     or d[off] is '\r' or '\n' (:463-470). Otherwise c is the first ':' in [off, L) -- the whole remainder, not the
 *     line (:475-477). With no c, or e exists and c >= e: name_len = size (the line end included) and no value
 *     (:479-484). Otherwise name_len = c - off and vp = c + 1; vp moves over bytes ' ' while vp < L; vp >= L before or
 *     after the skip means no value (:487-520); otherwise the value starts at vp and its length is L - vp with no e,
 *     else e - vp, less one when d[e-1] == '\r' (:521-538). With no '\n' the colon may lie behind the NUL that ended
 *     the field, so name_len can exceed size: that is kept.
 *   7 The walk (parseFields :87-139, getFieldCount :355-361, isHeaderComplete :412-426, getHeaderLen :436-439). The
 *     first field is at first_line_len and is linked always, at first_line_len == L too, where its size is 0. While
 *     the current field is not end-of-header and off + size < L: the field at off + size is read, and linked when its
 *     size is above 0; otherwise the walk ends. header_len is the last linked field's off + size; n_fields counts the
 *     linked fields that are not end-of-header; HEADER_COMPLETE is set when the last linked field is end-of-header or
 *     its name_len is 0 (isHeaderComplete compares getFieldName() with ""). The walk is linear in L: the position of
 *     the next ':' is carried from field to field and searched again only once it lies behind the new field's start.
 *   8 Names (:104-106, getFieldByName :395-410). A field's name bytes with 'A'..'Z' lowered, nothing else changed, are
 *     compared with spec->names[k] byte for byte; a trailing space before the colon is part of the name. FIRST is set
 *     on the first field of the message, in walk order, with a given name_id: the one getFieldByName returns. Records
 *     are emitted for no field, for the fields with a name_id, or for all non-end fields, by spec->fields.
 *   9 content_length, for both kinds (HttpLayer.cpp:728-737): the first non-end field whose lowered name is
 *     "content-length", whatever names[] holds. HAS_CONTENT_LENGTH is set when it exists. The number is atoi of its
 *     value cut at its first NUL, or of the empty text when it has no value: bytes of " \t\n\v\f\r" are skipped, then
 *     one optional sign, then digits. When the magnitude exceeds 2^31 - 1, CONTENT_LENGTH_RANGE is set and the number
 *     is 0 (atoi is undefined there).
 *  10 Text. A message's text is its `a` bytes (the URI / the status message) when spec->text bit 0 is set, then the
 *     value bytes of each emitted field that has a name_id and a value when bit 1 is set. text_len <= L, since the
 *     ranges are disjoint.
 *  11 Source bytes are read only inside [layer_offset, layer_offset + L) of in-bounds packets. */
#define PCPPX_HTTP_MAX_NAMES 8
#define PCPPX_HTTP_NAME_MAX 32

typedef struct pcppx_http_spec { /* 272 bytes */
	uint32_t max_msgs;  /* the HTTP packets the call has room for; 0 = n (always enough) */
	uint8_t kinds;      /* bit 0 requests, bit 1 responses; 1..3 */
	uint8_t fields;     /* PCPPX_HTTP_FIELDS_NONE (messages only), _WANTED (fields whose name is in names[]), _ALL */
	uint8_t text;       /* bit 0 PCPPX_HTTP_TEXT_FIRST_LINE (the URI / the status message), bit 1 PCPPX_HTTP_TEXT_VALUES
	                       (the values of wanted fields) */
	uint8_t n_names;    /* 0..8 */
	uint8_t name_len[PCPPX_HTTP_MAX_NAMES]; /* 1..32 for k < n_names, 0 beyond */
	char names[PCPPX_HTTP_MAX_NAMES][PCPPX_HTTP_NAME_MAX]; /* lower case already: no byte 'A'..'Z'; no two equal;
	                                                          unused bytes 0 */
} pcppx_http_spec;

#define PCPPX_HTTP_KIND_REQUESTS 1 /* pcppx_http_spec.kinds */
#define PCPPX_HTTP_KIND_RESPONSES 2
#define PCPPX_HTTP_FIELDS_NONE 0 /* pcppx_http_spec.fields */
#define PCPPX_HTTP_FIELDS_WANTED 1
#define PCPPX_HTTP_FIELDS_ALL 2
#define PCPPX_HTTP_TEXT_FIRST_LINE 1 /* pcppx_http_spec.text */
#define PCPPX_HTTP_TEXT_VALUES 2

#define PCPPX_HTTP_REQUEST 0 /* pcppx_http_msg.kind */
#define PCPPX_HTTP_RESPONSE 1
#define PCPPX_HTTP_METHOD_UNKNOWN 9  /* pcppx_http_msg.method: HttpMethod 0..8 (GET HEAD POST PUT DELETE TRACE OPTIONS
                                        CONNECT PATCH), else this */
#define PCPPX_HTTP_VERSION_UNKNOWN 3 /* pcppx_http_msg.version: HttpVersion 0 "0.9", 1 "1.0", 2 "1.1", else this */

/* pcppx_http_msg.flags */
#define PCPPX_HTTP_FIRST_LINE_COMPLETE 1   /* the first line's isComplete() */
#define PCPPX_HTTP_HEADER_COMPLETE 2       /* isHeaderComplete() */
#define PCPPX_HTTP_HAS_CONTENT_LENGTH 4    /* getFieldByName("content-length") finds a field */
#define PCPPX_HTTP_CONTENT_LENGTH_RANGE 8  /* its number does not fit an int: content_length is 0 */

/* pcppx_http_field.flags */
#define PCPPX_HTTP_HAS_VALUE 1 /* the field has a value (possibly of 0 bytes) */
#define PCPPX_HTTP_FIRST 2     /* getFieldByName(names[name_id]) returns this field */
#define PCPPX_HTTP_NO_NAME 0xFF /* pcppx_http_field.name_id of a name that is not in names[] */

typedef struct pcppx_http_msg { /* 48 bytes per HTTP packet, in source order */
	uint64_t first_field;    /* record number in out->fields of its first field record */
	uint64_t text_pos;       /* its first byte in out->text */
	uint32_t index;          /* source packet number (strictly ascending) */
	int32_t content_length;  /* getContentLength(), rule 9 */
	uint16_t layer_offset;   /* the HTTP layer's first byte, from the packet's first byte */
	uint16_t layer_len;      /* L */
	uint16_t header_len;     /* getHeaderLen() */
	uint16_t first_line_len; /* the first line's getSize() */
	uint16_t n_fields;       /* getFieldCount(), whatever spec->fields says */
	uint16_t n_rec;          /* the field records emitted for it */
	uint16_t a_offset;       /* request: the URI; response: the status message; from the layer's first byte */
	uint16_t a_len;          /* 0 with a_offset 0 when there is none */
	uint16_t status_code;    /* response: the number of rule 5, 0 = unknown; request: 0 */
	uint16_t text_len;       /* the bytes it put into out->text */
	uint8_t kind;            /* PCPPX_HTTP_REQUEST / PCPPX_HTTP_RESPONSE */
	uint8_t method;          /* request: HttpMethod 0..8 or 9; response: 9 */
	uint8_t version;         /* HttpVersion 0..2 or 3 */
	uint8_t flags;           /* PCPPX_HTTP_FIRST_LINE_COMPLETE | HEADER_COMPLETE | HAS_CONTENT_LENGTH | CONTENT_LENGTH_RANGE */
} pcppx_http_msg;

typedef struct pcppx_http_field { /* 24 bytes per emitted field, message by message, in walk order */
	uint64_t text_pos;     /* where its value lies (or would lie) in out->text */
	uint32_t msg;          /* its message's record number in out->msgs */
	uint16_t name_offset;  /* from the layer's first byte */
	uint16_t name_len;     /* getFieldName().size() */
	uint16_t value_offset; /* 0 with value_len 0 when the field has no value */
	uint16_t value_len;    /* getFieldValue().size() */
	uint16_t text_len;     /* value_len when its value went into out->text, else 0 */
	uint8_t name_id;       /* k with names[k] equal to the lower-cased name, else PCPPX_HTTP_NO_NAME */
	uint8_t flags;         /* PCPPX_HTTP_HAS_VALUE | PCPPX_HTTP_FIRST */
} pcppx_http_field;

/* pcppx_http_out.disposition values */
#define PCPPX_HTTP_NONE 0     /* no HTTP layer of a kind in spec->kinds that is followed (in bounds) */
#define PCPPX_HTTP_MSG 1      /* a message record */
#define PCPPX_HTTP_HOST 2     /* no recorded HTTP layer, but the host's chain may hold one (rule 3) */
#define PCPPX_HTTP_BAD_DESC 3 /* the descriptor is out of bounds: never read */

/* pcppx_http_out.totals words */
#define PCPPX_HTTP_MSGS 0
#define PCPPX_HTTP_REQUESTS 1
#define PCPPX_HTTP_RESPONSES 2
#define PCPPX_HTTP_FIELDS 3        /* the field records emitted */
#define PCPPX_HTTP_TEXT_BYTES 4
#define PCPPX_HTTP_HOST_N 5
#define PCPPX_HTTP_BAD_DESC_N 6
#define PCPPX_HTTP_HEADER_BYTES 7  /* the sum of header_len: HttpAnalyzer's totalMessageHeaderSize */
#define PCPPX_HTTP_FIELDS_LINKED 8 /* the sum of n_fields */
/* words 9 and 10 are zero */
#define PCPPX_HTTP_OVERFLOW 11
#define PCPPX_HTTP_TOTALS 12

typedef struct pcppx_http_out { /* device pointers; host pointers for pcppx_http_reference */
	pcppx_http_msg* msgs;     /* max_msgs entries, in source order */
	pcppx_http_field* fields; /* max_fields entries: message by message, each in walk order */
	uint8_t* text;            /* the messages' text back to back in record order, no terminator; NULL = no text */
	uint64_t text_cap;
	uint8_t* disposition;     /* optional (NULL): n entries, PCPPX_HTTP_* per source packet */
	uint32_t max_msgs;
	uint32_t max_fields;
	uint64_t* totals;         /* PCPPX_HTTP_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_http_out;

/* Capacity is all or nothing, as in dns: OVERFLOW = 1 iff MSGS > out->max_msgs, or FIELDS > max_fields, or text != NULL
 * and TEXT_BYTES > text_cap, or MSGS > spec->max_msgs (0 = n). Then only the totals are written (no record, no byte of
 * text, no disposition); they always hold the full would-be values. With text == NULL positions and lengths are still
 * filled and the byte capacity is not applied. Sizing: a call with max_msgs = max_fields = 0 overflows and gives MSGS,
 * FIELDS and TEXT_BYTES. The cost of a packet is linear in its layer's L bytes.
 * Source bytes are read only from in-bounds packets, inside a recorded HTTP layer that lies inside the packet. Nothing
 * is written outside the first MSGS messages, the first FIELDS records, [0, TEXT_BYTES) of text and the n dispositions.
 * The output is a pure function of the inputs, bit-identical from run to run: positions come from counts and scans, and
 * there are no atomics. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals, msgs or fields; with n > 0 a null
 * records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS; kinds 0 or above 3; fields above 2; text above 3; n_names above 8; a name_len of 0 or above 32 for
 * k < n_names, or not 0 beyond; a byte 'A'..'Z' in a name; two equal names. The work is queued on hip_stream and the
 * call returns without waiting; calls on one context are ordered through its http scratch (a buffer and an event of
 * their own, as dns's). Scratch: with g = ceil(n / 1024) blocks, 60 g + 16 n bytes (per block nine 32-bit sums -- its
 * messages, field records, text bytes, requests, responses, HOST and BAD_DESC packets, header bytes and linked
 * fields -- and the 64-bit exclusive prefixes of the first three; per packet a 16-byte plan: the layer's offset and
 * length, the kind, the records and text bytes of the message, its header length and linked fields, and the
 * disposition); PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_http_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                uint8_t max_layers, const pcppx_http_spec* spec, pcppx_http_out* out,
                                void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_http_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                   const pcppx_http_spec* spec, pcppx_http_out* out);

/* ---- ssl: the SSL/TLS records, the hellos and the SNI of the SSL packets of a device batch ----
 * What SSLStatsCollector::collectStats reads of a packet (Examples/SSLAnalyzer/SSLStatsCollector.h:141-401), for packets
 * that sit in HBM: per SSL packet one message record (the TCP payload size, the ports, the record-type mix), per
 * ClientHello / ServerHello one record (the versions, the cipher suite, the counts, the SNI host name's place), and the
 * host names back to back. Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * Inputs: as http. A device batch and its FIXED records (max_layers >= 1, the same value as the parse used; the summary
 * or, when it is NULL, the brief supplies flags and n_layers; PACKED and DENSE records are refused).
 *
 * Per packet i the first rule that applies decides (be16(x): the big-endian 16-bit word at byte x):
 *   1 BAD_DESC. offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (the rule of select, steer, defrag, frag,
 *     tlsfp, dns and http): the packet is never read.
 *   2 Incomplete chain: HOST when flags has PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC or DEPTH_OVERFLOW, or
 *     n_layers > max_layers, or NEEDS_HOST_L7 is set with L7_SSL set or without L7_KNOWN. The analyzer walks every SSL
 *     layer of the packet (SSLStatsCollector.h:319-375), so a chain the device did not record to its end is the host's
 *     even when some SSL entries were recorded: stricter than tlsfp's rule 3, on purpose.
 *   3 SSL entries. Every entry k < n_layers with proto == 18 (pcpp::SSL) that lies inside the packet (tlsfp's rule 2
 *     bounds: data_len >= 5, hdr_len >= 5, hdr_len <= data_len, offset + data_len <= caplen) is followed, in order; its
 *     record type is the byte at `offset`: 20 change-cipher-spec, 21 alert, 22 handshake, 23 application data
 *     (SSLLayer.cpp:42-94). An entry that fails the bounds is skipped and never read. No followed entry: NONE.
 *     Otherwise the packet is MSG and gets one message record. payload_len is the first followed entry's data_len
 *     (tcpLayer->getLayerPayloadSize(), SSLStatsCollector.h:276). Ports: with k0 the first followed entry, entry k0 - 1
 *     must have proto == 4 (pcpp::TCP) and offset + 4 <= caplen; then src_port = be16(offset) and dst_port =
 *     be16(offset + 2). Otherwise (k0 == 0 included) both ports are 0 and PCPPX_SSL_NO_TCP is set. ssl_port is src_port
 *     when SSLLayer::isSSLPort(src_port) holds (443, 261, 448, 465, 563, 614, 636, 989, 990, 992, 993, 994, 995;
 *     SSLLayer.h:488-510), else dst_port (SSLStatsCollector.h:291-296). n_handshake, n_ccs, n_alert and n_appdata count
 *     the followed entries by type, each saturating at 255; a followed entry of another type counts nowhere.
 *   4 Messages of a handshake entry (SSLLayer.cpp:126-150, SSLHandshake.cpp:1287-1350, 2257-2262). R = hdr_len - 5,
 *     cur = 0; loop: D = R - cur, stop when D < 4; the message starts at offset + 5 + cur. It is unknown, takes all of D
 *     and ends the walk when (a) D >= 16 and either its first five bytes are zero or its byte 1 is >= 1, or (b) its
 *     byte 0 is not one of 0, 1, 2, 4, 11, 12, 13, 14, 15, 16, 20: the default: of the switch at :1306-1332, whose
 *     SSLUnknownMessage::getMessageLength() is the whole rest. Otherwise its type is byte 0, M = min(4 + be16(2), D)
 *     and cur += M. The entry's ClientHello is the first message of type 1, its ServerHello the first of type 2
 *     (getHandshakeMessageOfType<>, SSLStatsCollector.h:353-364). One entry can yield both; they are emitted in ascending
 *     message offset, entry by entry. A kind that is not in spec->kinds is not emitted. (Case (b) is not in tlsfp's
 *     rule 4: there a hello behind a message of type 8 or 22 is still found; the reference does not find it.) Below,
 *     byte positions count from the message's first byte.
 *   5 Shared pieces: the session id, the cipher count and the extension list are rules 5-6 of tlsfp, the same reference
 *     functions. Field reads are bounded by D; the extension list is cut at M. n_ext is the number of extensions the
 *     list yields. header_version = D < 6 ? 0 : be16(4). session_id_len = sid.
 *   6 ClientHello record. version = header_version. n_ciphers is the count of tlsfp's rule 6; cipher is 0. SNI: the
 *     first listed extension of type 0, with data position x and length L (SSLHandshake.cpp:1138-1160, 1551-1575).
 *     None: no HAS_SNI. L == 0: HAS_SNI and an empty name (the reference returns "" and the analyzer counts it).
 *     L >= 5: the name is the bytes [x + 5, min(x + 5 + be16(x + 3), x + L)); SNI_TRUNCATED when the min cut it.
 *     1 <= L < 5: the reference reads the length word behind the extension and builds a string from an inverted range,
 *     which is undefined; here HAS_SNI | SNI_MALFORMED is set and the name is empty: a deliberate departure, as tlsfp's
 *     rule 7 has one.
 *   7 ServerHello record. version is tlsfp's rule 7: of the first listed extension of type 43, len == 2 gives
 *     be16(data), len == 3 with data[0] == 2 gives be16(data + 1); otherwise header_version (the len == 0 departure is
 *     kept). cipher = 39 + sid + 2 > D ? 0 : be16(39 + sid), with HAS_CIPHER when it is in bounds (getCipherSuiteID's
 *     isValid, SSLHandshake.cpp:1818-1830); whether the id is in the reference's name table is the host's concern.
 *     n_ciphers is 0. There is no SNI.
 *   8 Source bytes are read only inside followed SSL entries and the 4 port bytes, of in-bounds packets. */
typedef struct pcppx_ssl_spec {
	uint32_t max_msgs;   /* the SSL packets the call has room for; 0 = n (always enough) */
	uint8_t kinds;       /* bit 0 PCPPX_SSL_KIND_CLIENT, bit 1 PCPPX_SSL_KIND_SERVER; 0 = message records only */
	uint8_t reserved[3]; /* must be 0 */
} pcppx_ssl_spec;

#define PCPPX_SSL_KIND_CLIENT 1 /* pcppx_ssl_spec.kinds */
#define PCPPX_SSL_KIND_SERVER 2

#define PCPPX_SSL_CLIENT 1 /* pcppx_ssl_hello.kind */
#define PCPPX_SSL_SERVER 2

#define PCPPX_SSL_NO_TCP 1 /* pcppx_ssl_msg.flags: no TCP entry in front of the first followed SSL entry */

/* pcppx_ssl_hello.flags */
#define PCPPX_SSL_HAS_SNI 1       /* getExtensionOfType<SSLServerNameIndicationExtension>() finds one */
#define PCPPX_SSL_SNI_TRUNCATED 2 /* the name's length word reaches past the extension: cut there */
#define PCPPX_SSL_SNI_MALFORMED 4 /* 1 <= L < 5: the name is empty (rule 6) */
#define PCPPX_SSL_HAS_CIPHER 8    /* a ServerHello's cipher word lies inside D */

typedef struct pcppx_ssl_msg { /* 32 bytes per SSL packet, in source order */
	uint64_t first_hello;  /* record number in out->hellos of its first hello record */
	uint32_t index;        /* source packet number (strictly ascending) */
	uint32_t name_bytes;   /* the bytes its hellos put into out->names */
	uint16_t layer_offset; /* the first followed SSL entry's first byte, from the packet's first byte */
	uint16_t payload_len;  /* that entry's data_len: the TCP layer's payload size */
	uint16_t src_port;
	uint16_t dst_port;
	uint16_t ssl_port;     /* the port the analyzer's port table counts for a new flow */
	uint8_t n_handshake;   /* followed entries of type 22, saturating at 255; likewise the next three */
	uint8_t n_ccs;         /* type 20 */
	uint8_t n_alert;       /* type 21 */
	uint8_t n_appdata;     /* type 23 */
	uint8_t n_hellos;      /* the hello records emitted for it */
	uint8_t flags;         /* PCPPX_SSL_NO_TCP */
} pcppx_ssl_msg;

typedef struct pcppx_ssl_hello { /* 32 bytes per emitted hello: message by message, ascending msg_offset */
	uint64_t name_pos;       /* where its host name lies (or, with names == NULL, would lie) in out->names */
	uint32_t msg;            /* its message's record number in out->msgs */
	uint16_t msg_offset;     /* the hello message's first byte, from the packet's first byte */
	uint16_t name_len;       /* the host name's bytes; 0 without HAS_SNI */
	uint16_t version;        /* ClientHello: header_version; ServerHello: rule 7 (getHandshakeVersion) */
	uint16_t header_version;
	uint16_t cipher;         /* ServerHello: getCipherSuiteID(); ClientHello: 0 */
	uint16_t n_ciphers;      /* ClientHello: getCipherSuiteCount(); ServerHello: 0 */
	uint16_t n_ext;          /* getExtensionCount() */
	uint8_t kind;            /* PCPPX_SSL_CLIENT / PCPPX_SSL_SERVER */
	uint8_t layer;           /* the entry k it came from */
	uint8_t session_id_len;  /* getSessionIDLength() */
	uint8_t flags;           /* PCPPX_SSL_HAS_SNI | SNI_TRUNCATED | SNI_MALFORMED | HAS_CIPHER */
	uint8_t reserved[2];     /* written as 0 */
} pcppx_ssl_hello;

/* pcppx_ssl_out.disposition values */
#define PCPPX_SSL_NONE 0     /* a whole chain without a followed SSL entry */
#define PCPPX_SSL_MSG 1      /* a message record */
#define PCPPX_SSL_HOST 2     /* the chain was not recorded to its end (rule 2) */
#define PCPPX_SSL_BAD_DESC 3 /* the descriptor is out of bounds: never read */

/* pcppx_ssl_out.totals words */
#define PCPPX_SSL_MSGS 0
#define PCPPX_SSL_HELLOS 1
#define PCPPX_SSL_CLIENT_HELLOS 2
#define PCPPX_SSL_SERVER_HELLOS 3
#define PCPPX_SSL_NAME_BYTES 4
#define PCPPX_SSL_HOST_N 5
#define PCPPX_SSL_BAD_DESC_N 6
#define PCPPX_SSL_PAYLOAD_BYTES 7 /* the sum of payload_len: SSLAnalyzer's amountOfSSLTraffic */
#define PCPPX_SSL_ALERT_PKTS 8    /* messages with n_alert > 0 */
#define PCPPX_SSL_APPDATA_PKTS 9  /* messages with n_appdata > 0 */
/* word 10 is zero */
#define PCPPX_SSL_OVERFLOW 11
#define PCPPX_SSL_TOTALS 12

typedef struct pcppx_ssl_out { /* device pointers; host pointers for pcppx_ssl_reference */
	pcppx_ssl_msg* msgs;     /* max_msgs entries, in source order */
	pcppx_ssl_hello* hellos; /* max_hellos entries: message by message */
	uint8_t* names;          /* the host names back to back in record order, no terminator; NULL = positions only */
	uint64_t names_cap;
	uint8_t* disposition;    /* optional (NULL): n entries, PCPPX_SSL_* per source packet */
	uint32_t max_msgs;
	uint32_t max_hellos;
	uint64_t* totals;        /* PCPPX_SSL_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_ssl_out;

/* Capacity is all or nothing, as in http: OVERFLOW = 1 iff MSGS > out->max_msgs, or HELLOS > max_hellos, or
 * names != NULL and NAME_BYTES > names_cap, or MSGS > spec->max_msgs (0 = n). Then only the totals are written (no
 * record, no name byte, no disposition); they always hold the full would-be values. With names == NULL positions and
 * lengths are still filled and the byte capacity is not applied. Sizing: a call with max_msgs = max_hellos = 0
 * overflows (when there is an SSL packet) and gives MSGS, HELLOS and NAME_BYTES. The cost of a packet is linear in the
 * bytes of its handshake entries.
 * Source bytes are read only from in-bounds packets, inside followed SSL entries and the 4 port bytes. Nothing is
 * written outside the first MSGS messages, the first HELLOS hello records, [0, NAME_BYTES) of names and the n
 * dispositions. The output is a pure function of the inputs, bit-identical from run to run: positions come from counts
 * and scans, and there are no atomics. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: a null ctx, batch, records, spec, out, totals, msgs or hellos; with n > 0 a null
 * records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS; kinds above 3; a non-zero reserved byte. The work is queued on hip_stream and the call returns
 * without waiting; calls on one context are ordered through its ssl scratch (a buffer and an event of their own, as
 * http's). Scratch: with g = ceil(n / 1024) blocks, 64 g + 16 n bytes (per block ten 32-bit sums -- its messages, hello
 * records, name bytes, client and server hellos, HOST and BAD_DESC packets, payload bytes, alert and app-data packets --
 * and the 64-bit exclusive prefixes of the first three; per packet a 16-byte plan: its name bytes, its hello records,
 * the disposition and what the totals sum); PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_ssl_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                               uint8_t max_layers, const pcppx_ssl_spec* spec, pcppx_ssl_out* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_ssl_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                  const pcppx_ssl_spec* spec, pcppx_ssl_out* out);

/* ---- sip: the SIP messages, their header fields and their SDP bodies of a device batch ----
 * What SipRequestLayer / SipResponseLayer and the SdpLayer behind them give a VoIP monitor (Packet++/src/SipLayer.cpp,
 * SdpLayer.cpp, TextBasedProtocol.cpp), for packets that sit in HBM: per SIP packet one message record (the method or
 * the status code, the URI or the status text, header length, field count, content length), per header field the
 * caller asked for one record (Call-ID, From, To, CSeq ...), the bytes it asked for back to back, and per SDP body one
 * record (the owner address and the audio / video RTP ports). Added within ABI 7: new symbols only.
 *
 * The parse records hold no SIP layer: it runs the reference's four-byte SIP test (SipLayer::detectSipMessageType) and
 * the port test, flags the packet PCPPX_F_NEEDS_HOST_L7 and stops the chain at the L4 layer. So this operator restates
 * the reference's dispatch itself, from the recorded carrier (TCP / UDP) entry and the payload bytes.
 *
 * Inputs: as http. A device batch and its FIXED records (max_layers >= 1, the same value as the parse used; the summary
 * or, when it is NULL, the brief supplies flags and n_layers; PACKED and DENSE records are refused).
 *
 * Per packet i the first rule that applies decides. Positions count from the SIP layer's first byte (the carrier's
 * first payload byte); d[x] is the byte at x, L the payload length:
 *   1 BAD_DESC. offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (pcppx_move.h's out_of_bounds, as
 *     everywhere else): the packet is never read.
 *   2 Incomplete chain -> HOST: flags has PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC or DEPTH_OVERFLOW, or n_layers >
 *     max_layers, or NEEDS_HOST_L7 is set without L7_KNOWN (the VXLAN / GTP tunnels whose inner packet only the host
 *     parses).
 *   3 No candidate -> NONE: NEEDS_HOST_L7 is clear (the device built the whole chain: the reference builds a Payload
 *     there), or one of L7_HTTP / L7_SSL / L7_DNS is set (the device named another first L7 layer).
 *   4 The carrier: the last entry k < n_layers whose proto is 4 (pcpp::TCP) or 5 (pcpp::UDP). It must be the last
 *     entry, or be followed by one PacketTrailer (30) entry that is the last; it must lie inside the packet (8 <=
 *     hdr_len < data_len and offset + data_len <= caplen). Otherwise NONE. The payload is [offset + hdr_len, offset +
 *     data_len), L = data_len - hdr_len; the ports are the header's bytes 0..3 (big-endian source, destination).
 *   5 UDP, in UdpLayer::parseNextLayer's order (UdpLayer.cpp:103-183): the DHCP port pair (68->67, 67->68, 67->67) ->
 *     NONE; destination 4789 -> NONE; either port 5060 / 5061 -> the port path, rule 7. Otherwise the heuristic path:
 *     L < 4, or d[0..3] is none of the 15 keys "INVI" "ACK " "BYE " "CANC" "REGI" "PRAC" "OPTI" "SUBS" "NOTI" "PUBL"
 *     "INFO" "REFE" "MESS" "UPDA" "SIP/" (SipLayer.cpp:127-160) -> NONE. With a key, a port that gates a dissector of
 *     UdpLayer.cpp:122-165 -> HOST (whether that dissector takes the payload is the host's answer): either port 1812,
 *     1813, 3799 (RADIUS), 2152, 2123 (GTP), 546, 547 (DHCPv6), 123 (NTP), 13400, 3496 (DoIP), 30490 (SOME/IP's default
 *     port), 51820 (WireGuard), or destination 0, 7, 9 (WoL). Otherwise rule 8.
 *   6 TCP (TcpLayer.cpp:372-402; the HTTP and SSL branches ahead are excluded by rule 3): a port 5060 / 5061 on either
 *     side -> the port path, rule 7. Otherwise NONE: TCP has no heuristic.
 *   7 The port path (the six-argument SipLayer::parseSipLayer, SipLayer.cpp:162-184; TcpLayer.cpp:389-401). The
 *     method (SipRequestFirstLine::parseMethod :291-315) is the text before the first space, looked up among INVITE
 *     ACK BYE CANCEL REGISTER PRACK OPTIONS SUBSCRIBE NOTIFY PUBLISH INFO REFER MESSAGE UPDATE (0..13); it needs L >= 4
 *     and the space at 1..L-1. A known method -> a request. Otherwise the status code (parseStatusCode :1039-1054): L >=
 *     12, d[11] == ' ' and code = ((int8)d[8] - 48) * 100 + ((int8)d[9] - 48) * 10 + ((int8)d[10] - 48), the bytes
 *     sign-extended and the sum taken modulo 2^16 (parseStatusCodePure :695-705), is one of the 77 codes of the switch
 *     (:707-871). A known code -> a response; on UDP only when parseVersion (:1127-1146) is not empty too: L >= 8,
 *     d[0..3] == "SIP/" and a ' ' exists in [0, L). Otherwise NONE.
 *   8 The heuristic path (the four-argument parseSipLayer :186-209), via = 1. A request key: the method must be
 *     known, and SipRequestFirstLine::parseFirstLine (:317-393) must hold: with s1 the first space, a second space s2
 *     in (s1, L); s2 - s1 - 1 > 0 (the URI); with e the first '\r' or '\n' in (s2, L), else L, e - s2 - 1 >= 7; and
 *     d[s2+1..s2+4] == "SIP/". Otherwise NONE. The "SIP/" key (SipResponseFirstLine::parseFirstLine :1148-1196): L <
 *     12 -> NONE; s the first ' ' in [4, L), none -> NONE; the reference then reads d[s + 4] without a bound: with
 *     s + 4 >= L its answer is undefined and the packet is HOST; d[s + 4] != ' ' -> NONE; the code of d[s+1..s+3]
 *     (rule 7's arithmetic) unknown -> NONE; otherwise a response.
 *     A message whose kind is not in spec->kinds is NONE (HOST verdicts of rules 5 and 8 come first).
 *   9 A request's first line as the layer stores it (the constructor :213-246, parseVersion :395-433, getUri
 *     :479-489). u = len(method) + 1; v is the first " SIP/" in [u, L). With no v, or v + 7 > L, the version is
 *     unknown (m_VersionOffset = -1): there is no URI, and the '\n' that ends the line is searched from one byte
 *     before the layer -- the carrier header's last byte -- over L + 1 bytes. That is kept bit for bit: when that
 *     byte is 0x0A, first_line_len is 0 (and the line is complete); otherwise first_line_len is one past the first
 *     '\n' in [0, L), else L and not complete. The byte is in bounds by rule 4. With v, VERSION_KNOWN is set, the URI
 *     is [u, v), and with e the first '\n' in [v + 1, L) first_line_len = e + 1 (complete), else L (not complete).
 *  10 A response's first line (the constructor :1056-1079, getStatusCodeString :952-968). VERSION_KNOWN is rule 7's
 *     parseVersion. status_code is getStatusCodeAsInt() of rule 7's code when the version is known and the code is
 *     known, else 0: the code itself, but 425 for 423, 423 for 424 and 424 for 425, as the reference's
 *     StatusCodeEnumToInt (:687-692) lists those three in another order than its enum. That is kept.
 *     first_line_len is one past the first '\n' in [0, L) (complete), else L. With a status code the status text
 *     starts at 12 and ends at x = first_line_len - 2, or at x + 1 when d[x] != '\r'; a text that would end at or
 *     before 12 is empty (the reference's getStatusCodeString has no defined answer there).
 *  11 The fields: http's rules 6-8 exactly (the same parseFields, ':' as separator, spaces skipped), from
 *     first_line_len.
 *  12 content_length (SipLayer::getContentLength :57-66): http's rule 9 -- the first non-end field whose lowered name
 *     is "content-length". The compact name "l" is not recognised.
 *  13 SDP (SipLayer::parseNextLayer :85-110). HAS_SDP is set when L > header_len, content_length > 0 and the first
 *     non-end field whose lowered name is "content-type" has a value that contains the 15 bytes "application/sdp"
 *     (case-sensitive, std::string::find over all the value's bytes, NULs included). The body is [header_len, L); its
 *     fields are walked from its byte 0 as rule 11 walks, with '=' as the separator and no space skipped
 *     (SdpLayer.cpp:21-26, SdpLayer.h:156-163). Tokens are the value's runs of bytes other than " \t\n\v\f\r".
 *     Owner (getOwnerIPv4Address :74-95): the first field named "o" (one byte, 'O' too); it needs a value of >= 6
 *     tokens with token 3 == "IN" and token 4 == "IP4"; token 5, cut at its first NUL, is parsed as inet_pton(AF_INET)
 *     parses (IpAddress.cpp:63-69): four decimal numbers <= 255 of 1..3 digits, no leading zero before another digit,
 *     single dots between, nothing else. HAS_OWNER is set when the address parses and is not 0.0.0.0. Media
 *     (getMediaPort :97-114): the first field named "m" whose value has >= 2 tokens and token 0 == "audio" (resp.
 *     "video"): HAS_AUDIO (HAS_VIDEO), and the port is atoi of token 1 cut at its first NUL -- one optional sign, then
 *     digits, saturating at the 64-bit long's limits as strtol does -- cut to 16 bits.
 *  14 Source bytes are read only inside the carrier's payload of in-bounds packets, plus the carrier header's four
 *     port bytes and its last byte (rule 9). */
typedef pcppx_http_spec pcppx_sip_spec; /* 272 bytes, the same fields: max_msgs (0 = n); kinds (bit 0 requests, bit 1
                                           responses); fields (NONE / WANTED / ALL); text (bit 0 the URI / the status
                                           text, bit 1 the values of wanted fields); n_names <= 8 lower-case names of
                                           1..32 bytes, e.g. "call-id", "from", "to", "cseq" */
typedef pcppx_http_field pcppx_sip_field; /* 24 bytes: http's field record, offsets from the SIP layer's first byte */

#define PCPPX_SIP_REQUEST 0 /* pcppx_sip_msg.kind */
#define PCPPX_SIP_RESPONSE 1
#define PCPPX_SIP_METHOD_UNKNOWN 14 /* pcppx_sip_msg.method: SipMethod 0..13 (INVITE ACK BYE CANCEL REGISTER PRACK
                                       OPTIONS SUBSCRIBE NOTIFY PUBLISH INFO REFER MESSAGE UPDATE); a response: this */
#define PCPPX_SIP_VIA_PORT 0 /* pcppx_sip_msg.via: rule 7 */
#define PCPPX_SIP_VIA_HEURISTIC 1 /* rule 8 */

/* pcppx_sip_msg.flags */
#define PCPPX_SIP_FIRST_LINE_COMPLETE 1  /* the first line's isComplete() */
#define PCPPX_SIP_HEADER_COMPLETE 2      /* isHeaderComplete() */
#define PCPPX_SIP_HAS_CONTENT_LENGTH 4   /* getFieldByName("content-length") finds a field */
#define PCPPX_SIP_CONTENT_LENGTH_RANGE 8 /* its number does not fit an int: content_length is 0 */
#define PCPPX_SIP_VERSION_KNOWN 16       /* the first line's getVersion() is not empty */
#define PCPPX_SIP_HAS_SDP 32             /* an SdpLayer follows: one pcppx_sip_sdp record */
#define PCPPX_SIP_CARRIER_TCP 64         /* the carrier is TCP */

typedef struct pcppx_sip_msg { /* 48 bytes per SIP packet, in source order */
	uint64_t first_field;    /* record number in out->fields of its first field record */
	uint64_t text_pos;       /* its first byte in out->text */
	uint32_t index;          /* source packet number (strictly ascending) */
	int32_t content_length;  /* getContentLength(), rule 12 */
	uint16_t layer_offset;   /* the SIP layer's first byte, from the packet's first byte */
	uint16_t layer_len;      /* L */
	uint16_t header_len;     /* getHeaderLen() */
	uint16_t first_line_len; /* the first line's getSize() */
	uint16_t n_fields;       /* getFieldCount(), whatever spec->fields says */
	uint16_t n_rec;          /* the field records emitted for it */
	uint16_t a_offset;       /* request: the URI; response: the status text; from the layer's first byte */
	uint16_t a_len;          /* 0 with a_offset 0 when there is none */
	uint16_t status_code;    /* response: getStatusCodeAsInt(), 0 = unknown; request: 0 */
	uint16_t text_len;       /* the bytes it put into out->text */
	uint8_t kind;            /* PCPPX_SIP_REQUEST / PCPPX_SIP_RESPONSE */
	uint8_t method;          /* request: SipMethod 0..13; response: 14 */
	uint8_t via;             /* PCPPX_SIP_VIA_PORT / PCPPX_SIP_VIA_HEURISTIC */
	uint8_t flags;           /* PCPPX_SIP_* above */
} pcppx_sip_msg;

/* pcppx_sip_sdp.flags */
#define PCPPX_SIP_SDP_HAS_OWNER 1 /* getOwnerIPv4Address() != 0.0.0.0 */
#define PCPPX_SIP_SDP_HAS_AUDIO 2 /* an "m" field with >= 2 tokens and "audio" first exists */
#define PCPPX_SIP_SDP_HAS_VIDEO 4

typedef struct pcppx_sip_sdp { /* 32 bytes per message with HAS_SDP, in message order */
	uint32_t msg;          /* its message's record number in out->msgs */
	uint32_t index;        /* source packet number */
	uint16_t offset;       /* the body's first byte, from the SIP layer's first byte (= header_len) */
	uint16_t len;          /* L - header_len */
	uint16_t n_fields;     /* the SdpLayer's getFieldCount() */
	uint16_t audio_port;   /* getMediaPort("audio"); 0 without HAS_AUDIO */
	uint16_t video_port;   /* getMediaPort("video"); 0 without HAS_VIDEO */
	uint8_t flags;         /* PCPPX_SIP_SDP_* */
	uint8_t reserved0;     /* 0 */
	uint8_t owner_ipv4[4]; /* getOwnerIPv4Address(), network order; zeros without HAS_OWNER */
	uint8_t reserved[8];   /* 0 */
} pcppx_sip_sdp;

/* pcppx_sip_out.disposition values */
#define PCPPX_SIP_NONE 0     /* the reference builds no SIP layer of a kind in spec->kinds here */
#define PCPPX_SIP_MSG 1      /* a message record */
#define PCPPX_SIP_HOST 2     /* only the host can tell (rules 2, 5 and 8) */
#define PCPPX_SIP_BAD_DESC 3 /* the descriptor is out of bounds: never read */

/* pcppx_sip_out.totals words */
#define PCPPX_SIP_MSGS 0
#define PCPPX_SIP_REQUESTS 1
#define PCPPX_SIP_RESPONSES 2
#define PCPPX_SIP_FIELDS 3        /* the field records emitted */
#define PCPPX_SIP_TEXT_BYTES 4
#define PCPPX_SIP_HOST_N 5
#define PCPPX_SIP_BAD_DESC_N 6
#define PCPPX_SIP_HEADER_BYTES 7  /* the sum of header_len */
#define PCPPX_SIP_FIELDS_LINKED 8 /* the sum of n_fields */
#define PCPPX_SIP_SDPS 9          /* the SDP records emitted */
#define PCPPX_SIP_BY_HEURISTIC 10 /* messages with via == PCPPX_SIP_VIA_HEURISTIC */
#define PCPPX_SIP_OVERFLOW 11
#define PCPPX_SIP_TOTALS 12

typedef struct pcppx_sip_out { /* device pointers; host pointers for pcppx_sip_reference */
	pcppx_sip_msg* msgs;     /* max_msgs entries, in source order */
	pcppx_sip_field* fields; /* max_fields entries: message by message, each in walk order */
	pcppx_sip_sdp* sdps;     /* max_sdps entries, in message order */
	uint8_t* text;           /* the messages' text back to back in record order, no terminator; NULL = no text */
	uint64_t text_cap;
	uint8_t* disposition;    /* optional (NULL): n entries, PCPPX_SIP_* per source packet */
	uint32_t max_msgs;
	uint32_t max_fields;
	uint32_t max_sdps;
	uint32_t reserved;       /* 0 */
	uint64_t* totals;        /* PCPPX_SIP_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_sip_out;

/* Capacity is all or nothing, as in http: OVERFLOW = 1 iff MSGS > out->max_msgs, or FIELDS > max_fields, or SDPS >
 * max_sdps, or text != NULL and TEXT_BYTES > text_cap, or MSGS > spec->max_msgs (0 = n). Then only the totals are
 * written (no record, no byte of text, no disposition); they always hold the full would-be values. With text == NULL
 * positions and lengths are still filled and the byte capacity is not applied. Sizing: a call with max_msgs =
 * max_fields = max_sdps = 0 overflows (when there is a message) and gives MSGS, FIELDS, SDPS and TEXT_BYTES. The cost
 * of a packet is linear in its payload's L bytes.
 * Nothing is written outside the first MSGS messages, the first FIELDS records, the first SDPS records, [0,
 * TEXT_BYTES) of text and the n dispositions. The output is a pure function of the inputs, bit-identical from run to
 * run: positions come from counts and scans, and there are no atomics. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: http's list (a null ctx, batch, records, spec, out, totals, msgs or fields;
 * with n > 0 a null records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers
 * 0 or above PCPPX_MAX_LAYERS; kinds 0 or above 3; fields above 2; text above 3; n_names above 8; a name_len of 0 or
 * above 32 for k < n_names, or not 0 beyond; a byte 'A'..'Z' in a name; two equal names), plus a null sdps and a
 * non-zero out->reserved. The work is queued on hip_stream and the call returns without waiting; calls on one context
 * are ordered through its sip scratch (a buffer and an event of their own, as http's). Scratch: with g = ceil(n / 1024)
 * blocks, 76 g + 16 n bytes (per block eleven 32-bit sums -- its messages, field records, text bytes, SDP records,
 * requests, responses, HOST and BAD_DESC packets, header bytes, linked fields and heuristic-path messages -- and the
 * 64-bit exclusive prefixes of the first four; per packet a 16-byte plan: the layer's offset and length, the kind, the
 * path, the records and text bytes of the message, its header length and linked fields, whether it has an SDP body,
 * and the disposition); PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_sip_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                               uint8_t max_layers, const pcppx_sip_spec* spec, pcppx_sip_out* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_sip_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                  const pcppx_sip_spec* spec, pcppx_sip_out* out);

/* ---- dhcp: the DHCP and DHCPv6 messages and their options of a device batch ----
 * What DhcpLayer and DhcpV6Layer give passive asset discovery (Packet++/src/DhcpLayer.cpp, DhcpV6Layer.cpp, the option
 * walk of Packet++/header/TLVData.h's TLVRecordReader), for packets that sit in HBM: per DHCP / DHCPv6 packet one
 * message record (the BOOTP header's fields, the message type, the lease time, the server identifier, the option
 * count), per option the caller asked for one record, and the option values it asked for back to back. Both families
 * are option lists read by the same reader with two record shapes, so one operator covers both. Added within ABI 7:
 * new symbols only.
 *
 * The parse records hold no DHCP layer: it flags these packets PCPPX_F_NEEDS_HOST_L7 | PCPPX_F_L7_KNOWN and stops the
 * chain at the UDP layer. So this operator restates UdpLayer::parseNextLayer's dispatch (UdpLayer.cpp:103-141) itself,
 * from the recorded UDP entry and the ports.
 *
 * Inputs: as sip. A device batch and its FIXED records (max_layers >= 1, the same value as the parse used; the summary
 * or, when it is NULL, the brief supplies flags and n_layers; PACKED and DENSE records are refused).
 *
 * Per packet i the first rule that applies decides. Positions count from the layer's first byte (the UDP payload's
 * first byte); d[x] is the byte at x, L the payload length:
 *   1 BAD_DESC. offsets[i] + caplens[i] > data_len, the 64-bit wrap checked (pcppx_move.h's out_of_bounds): the packet
 *     is never read.
 *   2 Incomplete chain -> HOST: flags has PCPPX_F_NEEDS_HOST_PROTO, OVERSIZE, BAD_DESC or DEPTH_OVERFLOW, or n_layers >
 *     max_layers, or NEEDS_HOST_L7 is set without L7_KNOWN.
 *   3 No candidate -> NONE: NEEDS_HOST_L7 is clear, or one of L7_HTTP / L7_SSL / L7_DNS is set.
 *   4 The carrier: the last entry k < n_layers whose proto is 5 (pcpp::UDP). It must be the last entry, or be followed
 *     by one PacketTrailer (30) entry that is the last; hdr_len == 8 < data_len and offset + data_len <= caplen.
 *     Otherwise NONE; a TCP carrier is NONE. L = data_len - 8; the ports are the header's bytes 0..3 (big-endian source,
 *     destination).
 *   5 The DHCP port pair (68->67, 67->68, 67->67; DhcpLayer.h:784-788): L >= 240 (isDataValid :594-597) -> a DHCPv4
 *     message, whatever bytes 236..239 hold (the reference does not check the magic number); L < 240 -> NONE (the
 *     Payload fallback).
 *   6 Otherwise a DHCPv6 candidate needs a port 546 or 547 on either side; without one -> NONE. Destination port 4789,
 *     or a port 5060 / 5061 on either side -> NONE (VXLAN and SIP come first and both fall back to a Payload,
 *     UdpLayer.cpp:107-121). The other port one of 1812, 1813, 3799 (RADIUS), 2152, 2123 (GTP) -> HOST (whether that
 *     dissector takes the payload is the host's answer). L >= 4 (DhcpV6Layer.h:393-396) -> a DHCPv6 message; L < 4 ->
 *     NONE.
 *   7 A message whose family is not in spec->families is NONE (the HOST verdicts of rules 2 and 6 come first).
 *   8 The DHCPv4 options (getFirstTLVRecord / getNextTLVRecord over DhcpOption, DhcpLayer.h:452-492), from p = 240.
 *     At each step, with rem = L - p: rem < 1 stops. t = d[p]. t == 0 (PAD) or t == 255 (END): the record is one byte
 *     and its value length is 0. Otherwise rem < 2 stops; len = d[p + 1] and the record is 2 + len bytes. A record that
 *     ends behind L stops the walk and is not counted; otherwise it is counted and p moves behind it. END does not end
 *     the walk: trailing PAD bytes each count as an option, as getOptionsCount() counts them.
 *   9 The DHCPv6 options (DhcpV6Layer.cpp:37-51), from p = 4: L - p < 4 stops; code = be16(d[p]), len = be16(d[p + 2]),
 *     the record is 4 + len bytes; one that ends behind L stops the walk and is not counted. code is the two bytes as
 *     they are (DhcpV6Option::getType() maps codes outside its enum to 0; the record keeps the number).
 *  10 n_options is the count of rule 8 / 9 (getOptionsCount() / getOptionCount()) and options_len the bytes the counted
 *     records cover, whatever spec->options says. A record is emitted per counted option with spec->options ALL, and
 *     with WANTED per counted option whose code is wanted: bit c of want4 for DHCPv4 code c, a member of want6[0 ..
 *     n_codes6) for DHCPv6. With spec->values each emitted option's value bytes go to out->values, in walk order.
 *  11 Typed values, each from the first counted option of its code, whatever spec->options says. DHCPv4: msg_type is
 *     option 53's first value byte, 0 when the option is absent or its length is 0 (getMessageType,
 *     getValueAs<uint8_t>), HAS_MSG_TYPE when the option exists; lease_time is option 51's first four bytes big-endian
 *     when its length is >= 4, else 0, HAS_LEASE_TIME when the option exists with such a length; server_id is option
 *     54's first four bytes when its length is >= 4, else zeros, HAS_SERVER_ID likewise. client_mac is
 *     getClientHardwareAddress(): bytes 28..33 when htype == 1 and hlen == 6 (HAS_MAC), else zeros. MAGIC_OK: bytes
 *     236..239 are 63 82 53 63 (informational). REPLY: op == 2. DHCPv6: msg_type is d[0] when it is <= 13, else 0
 *     (DhcpV6Layer.cpp:83-92); xid is getTransactionID() (bytes 1..3, big-endian); the DHCPv4-only fields are zero.
 *  12 Source bytes are read only inside the UDP payload of in-bounds packets, plus the UDP header's four port bytes. */
typedef struct pcppx_dhcp_spec { /* 72 bytes */
	uint32_t max_msgs;   /* 0 = n */
	uint8_t families;    /* bit 0 DHCPv4, bit 1 DHCPv6; 1..3 */
	uint8_t options;     /* PCPPX_DHCP_OPTIONS_*: 0 NONE, 1 WANTED, 2 ALL (PAD / END included) */
	uint8_t values;      /* 1: the emitted options' value bytes go to out->values */
	uint8_t n_codes6;    /* <= PCPPX_DHCP_MAX_CODES6 */
	uint32_t want4[8];   /* bit c of the 256 (word c / 32, bit c % 32): DHCPv4 code c is wanted */
	uint16_t want6[16];  /* the wanted DHCPv6 codes, strictly ascending; 0 beyond n_codes6 */
} pcppx_dhcp_spec;
#define PCPPX_DHCP_V4 1 /* pcppx_dhcp_spec.families bits */
#define PCPPX_DHCP_V6 2
#define PCPPX_DHCP_OPTIONS_NONE 0
#define PCPPX_DHCP_OPTIONS_WANTED 1
#define PCPPX_DHCP_OPTIONS_ALL 2
#define PCPPX_DHCP_MAX_CODES6 16

typedef struct pcppx_dhcp_option { /* 16 bytes, message by message, in walk order */
	uint32_t msg;        /* its message's record number in out->msgs */
	uint16_t code;       /* getType(): d[p]; DHCPv6: be16(d[p]) */
	uint16_t len;        /* getDataSize() */
	uint16_t offset;     /* the record's first byte, from the layer's first byte */
	uint16_t ordinal;    /* its number among all the message's counted options */
	uint16_t value_rel;  /* its value's first byte in out->values, from the message's value_pos; 0 without values */
	uint16_t reserved;   /* 0 */
} pcppx_dhcp_option;

/* pcppx_dhcp_msg.flags */
#define PCPPX_DHCP_HAS_MSG_TYPE 1   /* option 53 was found */
#define PCPPX_DHCP_HAS_MAC 2        /* htype == 1 and hlen == 6 */
#define PCPPX_DHCP_MAGIC_OK 4       /* bytes 236..239 are 63 82 53 63 */
#define PCPPX_DHCP_HAS_LEASE_TIME 8 /* option 51 with a length >= 4 */
#define PCPPX_DHCP_HAS_SERVER_ID 16 /* option 54 with a length >= 4 */
#define PCPPX_DHCP_REPLY 32         /* op == 2 */

typedef struct pcppx_dhcp_msg { /* 80 bytes per DHCP / DHCPv6 packet, in source order */
	uint64_t first_option; /* record number in out->options of its first option record */
	uint64_t value_pos;    /* its first byte in out->values */
	uint32_t index;        /* source packet number (strictly ascending) */
	uint32_t xid;          /* DHCPv4: be32 of bytes 4..7; DHCPv6: getTransactionID() */
	uint32_t lease_time;   /* rule 11 */
	uint16_t layer_offset; /* the layer's first byte, from the packet's first byte */
	uint16_t layer_len;    /* L */
	uint16_t n_options;    /* getOptionsCount() / getOptionCount(), whatever spec->options says */
	uint16_t n_rec;        /* the option records emitted for it */
	uint16_t value_len;    /* the bytes it put into out->values */
	uint16_t options_len;  /* the bytes the counted options cover */
	uint16_t secs;         /* be16 of bytes 8..9 */
	uint16_t bootp_flags;  /* be16 of bytes 10..11 */
	uint8_t family;        /* 4 | 6 */
	uint8_t msg_type;      /* rule 11 */
	uint8_t flags;         /* PCPPX_DHCP_* above */
	uint8_t op;            /* getOpCode(): byte 0 */
	uint8_t htype, hlen, hops;
	uint8_t reserved0;     /* 0 */
	uint8_t ciaddr[4], yiaddr[4], siaddr[4], giaddr[4]; /* bytes 12..27, network order */
	uint8_t server_id[4];  /* rule 11 */
	uint8_t client_mac[6]; /* getClientHardwareAddress(): zeros unless htype 1, hlen 6 */
	uint8_t reserved[2];   /* 0 */
} pcppx_dhcp_msg;

/* pcppx_dhcp_out.disposition values */
#define PCPPX_DHCP_NONE 0     /* the reference builds no DHCP / DHCPv6 layer of a family in spec->families here */
#define PCPPX_DHCP_MSG 1      /* a message record */
#define PCPPX_DHCP_HOST 2     /* only the host can tell (rules 2 and 6) */
#define PCPPX_DHCP_BAD_DESC 3 /* the descriptor is out of bounds: never read */

/* pcppx_dhcp_out.totals words */
#define PCPPX_DHCP_MSGS 0
#define PCPPX_DHCP_V4_N 1
#define PCPPX_DHCP_V6_N 2
#define PCPPX_DHCP_OPTIONS 3        /* the option records emitted */
#define PCPPX_DHCP_VALUE_BYTES 4
#define PCPPX_DHCP_HOST_N 5
#define PCPPX_DHCP_BAD_DESC_N 6
#define PCPPX_DHCP_OPTIONS_LINKED 7 /* the sum of n_options */
#define PCPPX_DHCP_REPLIES 8        /* messages with PCPPX_DHCP_REPLY */
#define PCPPX_DHCP_OVERFLOW 9
#define PCPPX_DHCP_TOTALS 10

typedef struct pcppx_dhcp_out { /* device pointers; host pointers for pcppx_dhcp_reference */
	pcppx_dhcp_msg* msgs;       /* max_msgs entries, in source order */
	pcppx_dhcp_option* options; /* max_options entries: message by message, each in walk order */
	uint8_t* values;            /* the emitted options' values back to back in record order; NULL = no bytes */
	uint64_t values_cap;
	uint8_t* disposition;       /* optional (NULL): n entries, PCPPX_DHCP_* per source packet */
	uint32_t max_msgs;
	uint32_t max_options;
	uint64_t reserved;          /* 0 */
	uint64_t* totals;           /* PCPPX_DHCP_TOTALS words, overwritten by each call (not accumulated) */
} pcppx_dhcp_out;

/* Capacity is all or nothing, as in sip: OVERFLOW = 1 iff MSGS > out->max_msgs, or OPTIONS > max_options, or values !=
 * NULL and VALUE_BYTES > values_cap, or MSGS > spec->max_msgs (0 = n). Then only the totals are written (no record, no
 * value byte, no disposition); they always hold the full would-be values. With values == NULL positions and lengths
 * are still filled and the byte capacity is not applied. Sizing: a call with max_msgs = max_options = 0 overflows (when
 * there is a message) and gives MSGS, OPTIONS and VALUE_BYTES. The cost of a message is linear in its payload's L
 * bytes: the walk reads one or two bytes per option, and each emitted value byte is copied once.
 * Nothing is written outside the first MSGS messages, the first OPTIONS records, [0, VALUE_BYTES) of values and the n
 * dispositions. The output is a pure function of the inputs, bit-identical from run to run: positions come from counts
 * and scans, and there are no atomics. n == 0 is legal (zero totals).
 * PCPPX_E_INVAL before any device work: sip's list (a null ctx, batch, records, spec, out, totals or msgs; with n > 0 a
 * null records->layers, or records->summary and records->brief both; PACKED or DENSE records; max_layers 0 or above
 * PCPPX_MAX_LAYERS), plus families 0 or above 3; options above 2; values above 1; n_codes6 above 16; want6 not strictly
 * ascending below n_codes6, or not 0 beyond; a null out->options; a non-zero out->reserved. The work is queued on
 * hip_stream and the call returns without waiting; calls on one context are ordered through its dhcp scratch (a buffer
 * and an event of their own, as sip's). Scratch: with g = ceil(n / 1024) blocks, 60 g + 16 n bytes (per block nine
 * 32-bit sums -- its messages, option records, value bytes, DHCPv4 and DHCPv6 messages, HOST and BAD_DESC packets,
 * linked options and replies -- and the 64-bit exclusive prefixes of the first three; per packet a 16-byte plan: the
 * layer's offset and length, the family, the records and value bytes of the message, its option count, whether it is a
 * reply, and the disposition); PCPPX_E_NOMEM when it cannot be allocated. */
PCPPX_API int pcppx_dhcp_device(pcppx_ctx* ctx, const pcppx_batch* batch, const pcppx_records* records,
                                uint8_t max_layers, const pcppx_dhcp_spec* spec, pcppx_dhcp_out* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. */
PCPPX_API int pcppx_dhcp_reference(const pcppx_batch* batch, const pcppx_records* records, uint8_t max_layers,
                                   const pcppx_dhcp_spec* spec, pcppx_dhcp_out* out);

/* ---- bpf: classic BPF filter programs run over the packets of a device batch (the capture-side filter step) ----
 * The reference's users choose packets with pcap filters: IFileReaderDevice::setFilter,
 * BpfFilterWrapper::matchPacketWithFilter and the GeneralFilter family (Pcap++/src/PcapFilter.cpp) all end in
 * pcap_offline_filter over a compiled bpf_program with len = caplen (PcapFilter.cpp:122-127). The compiler stays with
 * the caller (libpcap's pcap_compile); this is the interpreter, as a kernel: one or several validated programs run over
 * every packet of a batch in HBM, with no parse, and the verdicts come out as the columns select and steer consume:
 * matched[] is pcppx_select_spec.keep, bucket[] (the first accepting program; 0xFF = none, i.e. >= n_buckets = not
 * steered) is pcppx_steer_spec.bucket. Added within ABI 7: new symbols only (PCPPX_ABI_VERSION stays 7).
 *
 * The machine is libpcap's userland bpf_filter with no auxiliary data, per packet i:
 *   state    A, X and M[0..15] are 32-bit and start at zero for every program; buflen = caplens[i]; wirelen =
 *            frame_lens[i], or caplens[i] when frame_lens is NULL (the reference's own call, PcapFilter.cpp:124-125).
 *   ld abs   LD|W|ABS, LD|H|ABS, LD|B|ABS: A = the big-endian 4 / 2 / 1 bytes at k. The packet is rejected (the program
 *            returns 0) when k > buflen || size > buflen - k (for B: k >= buflen).
 *   ld ind   LD|W|IND, LD|H|IND, LD|B|IND: the same at X + k; rejected when k > buflen || X > buflen - k ||
 *            size > buflen - (X + k): nothing wraps 32 bits.
 *   ldx msh  LDX|B|MSH: X = (P[k] & 0xf) << 2, bounded as the B load.
 *   others   LD|IMM (A = k), LD|MEM (A = M[k]), LD|W|LEN (A = wirelen), LDX|W|IMM, LDX|W|MEM, LDX|W|LEN the same
 *            into X; ST (M[k] = A), STX (M[k] = X).
 *   alu      ALU|ADD, SUB, MUL, DIV, MOD, AND, OR, XOR, LSH, RSH with K or X as the operand, modulo 2^32; DIV or MOD
 *            by X == 0 rejects the packet; a shift by 32 or more gives 0. ALU|NEG: A = -A.
 *   jumps    JMP|JA: pc += k. JMP|JEQ, JGT, JGE, JSET with K or X: pc += (condition ? jt : jf); unsigned comparisons;
 *            JSET tests A & operand.
 *   rest     RET|K returns k, RET|A returns A; MISC|TAX (X = A), MISC|TXA (A = X).
 * A packet of any caplen (0, or above PCPPX_MAX_CAPLEN) is filtered: BPF is not a parse. batch->linktype is ignored
 * (it mattered when the program was compiled). eBPF, the Linux SKF_AD_* ancillary offsets and auxiliary VLAN data are
 * out of scope: such offsets are ordinary out-of-range loads and reject, as in pcap_offline_filter.
 *
 * Validation (pcppx_bpf_validate; pcppx_bpf_load applies it per program), PCPPX_E_INVAL otherwise:
 * 1 <= n_insns <= PCPPX_BPF_MAX_INSNS; every opcode is one of those above; a MEM / ST / STX index is below
 * PCPPX_BPF_MEMWORDS; DIV or MOD by a constant 0 is refused; for JA, i + 1 + k does not wrap and is < n_insns; for the
 * conditional jumps i + 1 + jt and i + 1 + jf are < n_insns; the last instruction is a RET. Jumps go forward only, so
 * every program ends within n_insns steps. */
typedef struct pcppx_bpf_insn { /* layout of struct bpf_insn / sock_filter: a bpf_program's bf_insns can be passed as is */
	uint16_t code;
	uint8_t jt, jf;
	uint32_t k;
} pcppx_bpf_insn;
#define PCPPX_BPF_MAX_INSNS 4096   /* per program (BPF_MAXINSNS) */
#define PCPPX_BPF_MAX_PROGRAMS 16
#define PCPPX_BPF_MEMWORDS 16
typedef struct pcppx_bpf_prog { /* host memory */
	const pcppx_bpf_insn* insns;
	uint32_t n_insns;
	uint32_t reserved;
} pcppx_bpf_prog;
typedef struct pcppx_bpf pcppx_bpf; /* validated programs resident on a context's GPU */

/* pcppx_bpf_verdicts.totals words */
#define PCPPX_BPF_MATCHED 0  /* packets some program accepted */
#define PCPPX_BPF_BAD_DESC 1 /* offsets[i] + caplens[i] > data_len (or wraps 64 bits): never read, rejected */
#define PCPPX_BPF_TOTALS 8   /* words 2-7 zero */
typedef struct pcppx_bpf_verdicts { /* device pointers for _device, host for _reference; each column may be NULL */
	uint8_t* matched; /* n: 1 iff some program returns non-zero, else 0 (select's keep[]) */
	uint8_t* bucket;  /* n: index of the first program (in load order) that returns non-zero, else 0xFF (steer's column) */
	uint32_t* ret;    /* n: that program's return value (bpf_filter's result: the snap length), else 0 */
	uint64_t* totals; /* required: PCPPX_BPF_TOTALS words, overwritten by each call */
} pcppx_bpf_verdicts;

/* The validation rules above over one program in host memory; PCPPX_OK or PCPPX_E_INVAL. Host only, no GPU. */
PCPPX_API int pcppx_bpf_validate(const pcppx_bpf_insn* insns, uint32_t n_insns);
/* Validate n_progs (1..PCPPX_BPF_MAX_PROGRAMS) programs and copy them, back to back in load order, into one buffer on
 * ctx's GPU. The handle is independent of the caller's arrays afterwards; it may be used by any number of calls. */
PCPPX_API int pcppx_bpf_load(pcppx_ctx* ctx, const pcppx_bpf_prog* progs, uint32_t n_progs, pcppx_bpf** out);
PCPPX_API void pcppx_bpf_free(pcppx_bpf* f); /* waits for queued work that uses f */
/* Run f's programs, in load order, over every packet of a device batch (frame_lens: device, n entries, or NULL); a
 * packet's verdict is that of the first program that returns non-zero (later programs are not run for it). A packet
 * with a bad descriptor gets matched 0, bucket 0xFF, ret 0 and counts in PCPPX_BPF_BAD_DESC; its bytes are never read.
 * Only the first n entries of each non-NULL column are written. Source bytes are read only through aligned 4-byte
 * words that hold at least one byte of an in-bounds packet. The output is a pure function of the inputs; the totals are
 * integer counts. PCPPX_E_INVAL before any device work: a null ctx, f, batch, out or totals. n == 0 is legal and
 * writes zero totals. The work is queued on hip_stream and the call returns without waiting (the totals stay on the
 * device); calls share no scratch, so calls on different streams may overlap. */
PCPPX_API int pcppx_bpf_device(pcppx_ctx* ctx, const pcppx_bpf* f, const pcppx_batch* batch, const uint32_t* frame_lens,
                               pcppx_bpf_verdicts* out, void* hip_stream);
/* The same contract in plain C++ over host pointers (no GPU, no context): what a host caller uses. PCPPX_E_INVAL: a
 * null progs, insns pointer, batch, out or totals; n_progs 0 or above PCPPX_BPF_MAX_PROGRAMS; a non-zero reserved
 * field; a program that does not validate (pcppx_bpf_load refuses the same). */
PCPPX_API int pcppx_bpf_reference(const pcppx_bpf_prog* progs, uint32_t n_progs, const pcppx_batch* batch,
                                  const uint32_t* frame_lens, pcppx_bpf_verdicts* out);

/* ---- host ingest: pcap / pcapng captures into packed batch buffers ---- */
typedef struct pcppx_pcap pcppx_pcap;
/* Open a capture; the format comes from its first 4 bytes as IFileReaderDevice::createReader
 * (Pcap++/src/PcapFileDevice.cpp:546-583): pcap as PcapFileReaderDevice::open (:707-768, incl. its version
 * and snapshot-length checks), pcapng as PcapNgFileReaderDevice::open (:1157-1176, LightPcapNg). */
PCPPX_API int pcppx_pcap_open(const char* path, pcppx_pcap** out);
/* RawPacket::getLinkLayerType of the packets of the last batch returned (before the first batch: of the
 * first packet). pcap: the file header's, LINKTYPE_INVALID (0xFFFF) outside LinkLayerType; pcapng: the
 * packet's interface's. */
PCPPX_API uint32_t pcppx_pcap_linktype(const pcppx_pcap* reader);
/* Append up to max_packets records back to back into data[0, data_cap) (pinned memory feeds
 * pcppx_parse_batch_host without a staging copy); *n_out = packets read (0 at end of file). Record checks
 * as PcapFileReaderDevice::readNextPacket (PcapFileDevice.cpp:799-886) / light_get_next_packet. A batch
 * holds one link type: it ends before a packet of another (pcapng interfaces). timestamps_ns may be NULL. */
PCPPX_API int pcppx_pcap_read_batch(pcppx_pcap* reader, uint8_t* data, uint64_t data_cap, uint64_t* offsets,
                          uint32_t* caplens, uint64_t* timestamps_ns, uint32_t max_packets, uint32_t* n_out,
                          uint64_t* bytes_out);
/* as pcppx_pcap_read_batch, plus each packet's original (wire) length, RawPacket::getFrameLength
 * (frame_lens may be NULL) */
PCPPX_API int pcppx_pcap_read_batch_ex(pcppx_pcap* reader, uint8_t* data, uint64_t data_cap, uint64_t* offsets,
                          uint32_t* caplens, uint32_t* frame_lens, uint64_t* timestamps_ns, uint32_t max_packets,
                          uint32_t* n_out, uint64_t* bytes_out);
/* Zero-copy: the next batch's packets stay where they are in the reader's memory-mapped file. *data = the map
 * base, *data_len = the file size, offsets[i] = the position of packet i's bytes in it (caplens / frame_lens /
 * timestamps_ns as pcppx_pcap_read_batch_ex; the same records and batch boundaries). The file's record headers lie
 * between the packets -- a gapped, ascending batch, which pcppx_parse_batch_host stages as near-contiguous ranges.
 * The bytes stay valid until pcppx_pcap_close. */
PCPPX_API int pcppx_pcap_map_batch(pcppx_pcap* reader, const uint8_t** data, uint64_t* data_len, uint64_t* offsets,
                                   uint32_t* caplens, uint32_t* frame_lens, uint64_t* timestamps_ns, uint32_t max_packets,
                                   uint32_t* n_out);
PCPPX_API void pcppx_pcap_close(pcppx_pcap* reader);

/* PCPPX_LAYOUT_PACKED layer entries (host memory, from a device parse) -> the FIXED layout: fixed[i * max_layers + k]
 * for k < min(summary[i].n_layers, max_layers), zero past each chain. max_layers <= PCPPX_PACKED_MAX_LAYERS. */
PCPPX_API int pcppx_unpack_layers(const pcppx_summary* summary, const pcppx_layer* packed, uint64_t n,
                                  uint32_t max_layers, pcppx_layer* fixed);
/* the same with the chain lengths from briefs (ABI 7) */
PCPPX_API int pcppx_unpack_layers_brief(const pcppx_brief* brief, const pcppx_layer* packed, uint64_t n,
                                        uint32_t max_layers, pcppx_layer* fixed);
PCPPX_API void* pcppx_host_alloc(size_t bytes); /* page-locked host memory (hipHostMalloc) */
PCPPX_API void pcppx_host_free(void* p);

#ifdef __cplusplus
}
#endif

#endif /* PCPPX_H */
