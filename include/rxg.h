/*
 * rxg.h — C ABI of the MI355X-native receive-path engine ("rxg").
 *
 * rxg replaces the per-packet receive stage of rajneshrat/dpdk-tcpipstack:
 *
 *   l2fwd_main_loop: for (i < nb_rx) ether_in(pkts[i])      tcp_ip_stack/main.c:396-399
 *     ether_in   -> switch ether_type                       tcp_ip_stack/etherin.c:12-37
 *     ip_in      -> ARP learn, proto==6 -> tcp_in           tcp_ip_stack/ip.c:19-42
 *     tcp_in     -> findtcb, RST verdicts, tcpswitch[state]  tcp_ip_stack/tcp_in.c:32-84
 *     findtcb    -> two-pass linear 4-tuple / listener scan tcp_ip_stack/tcp_tcb.c:127-173
 *     calculate_checksum (RFC 1071 byte loop)               tcp_ip_stack/ip.c:44-59
 *
 * with one batched, device-resident pass on gfx950 (parse + IPv4 header checksum +
 * TCP pseudo-header checksum + 4-tuple -> TCB classify), followed by an in-order host
 * replay that performs exactly the side effects the reference performs
 * (free_mbuf, send_reset, ARP learn, max_seq_received, AdjustSendWindow,
 * tcpswitch[state]).
 *
 * Conventions
 *  - Every entry point returns 0 on success or a negative errno-style code
 *    (-EINVAL, -ENOMEM, -EIO for a HIP runtime error, -ENODEV without a GPU).
 *    Nothing asserts; nothing falls back to a CPU path.
 *  - Plain pointers and sizes only.  "dev" pointers are HIP device pointers.
 *  - A `stream` argument is a hipStream_t passed as void*; NULL = the context's own stream.
 *  - Field byte orders follow the reference exactly (see rxg_rec48 below).
 */
#ifndef RXG_H
#define RXG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RXG_ABI_VERSION 2

/* ------------------------------------------------------------------------- */
/* Protocol constants (wire formats; reference names in comments).            */
/* ------------------------------------------------------------------------- */
#define RXG_ETHER_TYPE_IPV4 0x0800 /* ETHER_TYPE_IPv4, etherin.c:28 */
#define RXG_ETHER_TYPE_ARP  0x0806 /* ETHER_TYPE_ARP,  etherin.c:22 */
#define RXG_IPPROTO_TCP     6      /* IPPROTO_TCP,     ip.c:29      */

/* TCP_FLAGS, tcp_ip_stack/tcp.h:12-21 */
#define RXG_TCP_FLAG_FIN 0x01
#define RXG_TCP_FLAG_SYN 0x02
#define RXG_TCP_FLAG_RST 0x04
#define RXG_TCP_FLAG_PSH 0x08
#define RXG_TCP_FLAG_ACK 0x10

/* enum TCP_STATE_, tcp_ip_stack/tcp_states.h:8-17 */
enum rxg_tcp_state {
    RXG_TCP_STATE_CLOSED = 0,
    RXG_LISTENING = 1,
    RXG_SYN_SENT = 2,
    RXG_SYN_RECV = 3,
    RXG_TCP_ESTABLISHED = 4,
    RXG_TCP_STATE_FIN_1 = 5,
    RXG_TCP_FIN_2 = 6,
    RXG_TCP_STATES = 7
};
#define RXG_STATE_NONE 0xFF /* no TCB chosen */

/* Fixed offsets the reference uses regardless of IHL (tcp_in.c:42-45). */
#define RXG_OFF_IP  14
#define RXG_OFF_TCP 34

/* Reference table capacity (TOTAL_TCBS, tcp_tcb.c:16). rxg itself has no such cap. */
#define RXG_REF_TOTAL_TCBS 20000

/* ------------------------------------------------------------------------- */
/* Per-packet result records.                                                 */
/* ------------------------------------------------------------------------- */

/* What the reference does with the packet (the branch ether_in/ip_in/tcp_in take). */
enum rxg_verdict {
    RXG_V_DISPATCH = 0,          /* tcpswitch[state](tcb, tcp, ip, m)   tcp_in.c:65-72     */
    RXG_V_RST_NOPCB = 1,         /* ++tcpnopcb; free; send_reset        tcp_in.c:47-53     */
    RXG_V_RST_LISTEN_NONSYN = 2, /* LISTENING && !SYN: free; send_reset tcp_in.c:54-59     */
    RXG_V_DROP_NONTCP = 3,       /* IPv4, next_proto_id != 6: free      ip.c:36-39         */
    RXG_V_ARP = 4,               /* arp_in(m); free_mbuf(m)             etherin.c:22-27    */
    RXG_V_DROP_L2 = 5            /* other ether_type: free_mbuf         etherin.c:33-34    */
};

/* rxg_rec16.flags bits */
enum rxg_rec_flag {
    RXG_F_IP_OK = 0x01,        /* IPv4 and ip_cksum == 0                                     */
    RXG_F_TCP_OK = 0x02,       /* TCP and tcp_cksum == 0                                     */
    RXG_F_LISTEN = 0x04,       /* TCB found by findtcb pass 2 (listener on dport)            */
    RXG_F_REF_NULLSLOT = 0x08, /* pass 2 met a removed (NULL) slot before its answer: the
                                  reference dereferences NULL there (tcp_tcb.c:160-162);
                                  rxg skips the slot and reports it                        */
    RXG_F_TRUNC = 0x10,        /* frame shorter than the 54 bytes the path reads; bytes at
                                  and beyond data_len are read as zero                      */
    RXG_F_ARP_LEARN = 0x20     /* TCP packet whose host-order source IP is not in the ARP
                                  mirror as of the burst: ip.c:30-32 would call add_mac
                                  unless an earlier packet of the burst already added it
                                  (only computed while the ARP mirror is enabled)           */
};

/*
 * 16-byte compact record: everything the in-order host replay needs that is not a
 * plain re-read of the (host-resident) frame.
 */
typedef struct rxg_rec16 {
    int32_t tcb_idx;    /* index into tcbs[] chosen by findtcb (tcp_tcb.c:127-173); -1 = NULL */
    uint16_t ip_cksum;  /* calculate_checksum(frame+14, 20); 0x0000 = header valid             */
    uint16_t tcp_cksum; /* calculate_checksum(pseudo || frame[34 .. 14+total_length));
                           pseudo = {src_addr, dst_addr, 0, 6, htons(total_length-20)}
                           exactly as ip_out builds it (ip.c:109-118); 0x0000 = valid          */
    uint8_t verdict;    /* enum rxg_verdict                                                     */
    uint8_t state;      /* tcbs[tcb_idx]->state at classify time, RXG_STATE_NONE if none        */
    uint8_t tcp_flags;  /* frame byte 47                                                        */
    uint8_t flags;      /* enum rxg_rec_flag                                                    */
    int32_t datalen;    /* ntohs(total_length) - (version_ihl&0xf)*4 - (data_off>>4)*4
                           as the state handlers compute it (tcp_states.c:48-50,103-111)       */
} rxg_rec16;

/* 48-byte full record: the compact record plus every header field the path extracts. */
typedef struct rxg_rec48 {
    rxg_rec16 c;          /* bytes 0..15                                                  */
    uint16_t ether_type;  /* 16: ntohs(eth->ether_type)                 etherin.c:21        */
    uint16_t sport;       /* 18: ntohs(tcp->src_port)                   tcp_tcb.c:135       */
    uint16_t dport;       /* 20: ntohs(tcp->dst_port)                   tcp_tcb.c:134       */
    uint8_t l4_proto;     /* 22: ip->next_proto_id                      ip.c:28             */
    uint8_t version_ihl;  /* 23: ip->version_ihl                        tcp_states.c:49     */
    uint32_t seq;         /* 24: ntohl(tcp->sent_seq)                   tcp_in.c:66         */
    uint32_t ack;         /* 28: ntohl(tcp->recv_ack)                   tcp_in.c:71         */
    uint32_t src_ip;      /* 32: ntohl(ip->src_addr), host order        ip.c:30, tcp_tcb.c:155 */
    uint32_t dst_ip_raw;  /* 36: ip->dst_addr as loaded (network order) tcp_tcb.c:154       */
    uint8_t data_off;     /* 40: tcp->data_off (raw byte 46)            tcp_states.c:48     */
    uint8_t src_mac[6];   /* 41: eth->s_addr                            ip.c:31             */
    uint8_t reserved;     /* 47: 0                                                          */
} rxg_rec48;
/* total_length = c.datalen + (version_ihl & 0xf) * 4 + (data_off >> 4) * 4. */

/* 8-byte record (RXG_REC8): what rxg_rx_replay and rxg_payload_gather_dev use, half the
   bytes of rxg_rec16 per frame; the two checksums are carried as RXG_F_IP_OK /
   RXG_F_TCP_OK only.
     w0  bits  0-23  tcb_idx + 1 (0: findtcb returned NULL)
         bits 24-26  verdict (enum rxg_verdict)
         bits 27-29  state (7: RXG_STATE_NONE)
     w1  bits  0-7   tcp_flags
         bits  8-13  flags (enum rxg_rec_flag)
         bits 14-30  datalen + 128 (datalen >= -120: total_length - 60 - 60)           */
typedef struct rxg_rec8 {
    uint32_t w0, w1;
} rxg_rec8;

enum rxg_rec_kind { RXG_REC8 = 8, RXG_REC16 = 16, RXG_REC48 = 48 };

/* rxg_rec8 -> rxg_rec16.  A checksum the record only knows as "not 0x0000" reads 0xFFFF
   (IPv4 frames without RXG_F_IP_OK, TCP segments without RXG_F_TCP_OK); the others 0. */
static inline void rxg_rec8_expand(const rxg_rec8 *r, rxg_rec16 *o)
{
    const uint32_t v = (r->w0 >> 24) & 7u, st = (r->w0 >> 27) & 7u, fl = (r->w1 >> 8) & 0x3Fu;
    const int ip = v <= RXG_V_DROP_NONTCP, tcp = v <= RXG_V_RST_LISTEN_NONSYN;
    o->tcb_idx = (int32_t)(r->w0 & 0xFFFFFFu) - 1;
    o->ip_cksum = (uint16_t)((ip && !(fl & RXG_F_IP_OK)) ? 0xFFFFu : 0u);
    o->tcp_cksum = (uint16_t)((tcp && !(fl & RXG_F_TCP_OK)) ? 0xFFFFu : 0u);
    o->verdict = (uint8_t)v;
    o->state = (uint8_t)(st == 7u ? RXG_STATE_NONE : st);
    o->tcp_flags = (uint8_t)(r->w1 & 0xFFu);
    o->flags = (uint8_t)fl;
    o->datalen = (int32_t)((r->w1 >> 14) & 0x1FFFFu) - 128;
}

/* ------------------------------------------------------------------------- */
/* Per-GPU counters (merged across GPUs with an RCCL all-reduce, sum, uint64). */
/* ------------------------------------------------------------------------- */
enum rxg_counter {
    RXG_C_RX = 0,           /* frames seen                                            */
    RXG_C_BYTES,            /* sum of data_len                                        */
    RXG_C_IPV4,             /* ether_type 0x0800                                      */
    RXG_C_ARP,              /* ether_type 0x0806                                      */
    RXG_C_OTHER_L2,         /* any other ether_type                                   */
    RXG_C_TCP,              /* IPv4 with next_proto_id 6                              */
    RXG_C_NON_TCP,          /* IPv4, other protocol                                   */
    RXG_C_IP_CKSUM_BAD,     /* IPv4 with ip_cksum != 0                                */
    RXG_C_TCP_CKSUM_BAD,    /* TCP with tcp_cksum != 0 (tcpchecksumerror, tcp_in.c:18) */
    RXG_C_TCB_HIT_EXACT,    /* findtcb pass 1 hit                                     */
    RXG_C_TCB_HIT_LISTEN,   /* findtcb pass 2 hit                                     */
    RXG_C_NOPCB,            /* findtcb NULL (tcpnopcb, tcp_in.c:48)                   */
    RXG_C_LISTEN_NONSYN,    /* RST to a non-SYN on a listener                         */
    RXG_C_DISPATCH,         /* handed to tcpswitch[state]                             */
    RXG_C_REF_NULLSLOT,     /* reference would have dereferenced a NULL slot          */
    RXG_C_TRUNC,            /* frames shorter than 54 bytes                           */
    RXG_NCOUNTERS
};

/* ------------------------------------------------------------------------- */
/* Context                                                                    */
/* ------------------------------------------------------------------------- */
typedef struct rxg_ctx rxg_ctx;

typedef struct rxg_config {
    int32_t device;        /* HIP device ordinal (one context per GPU, one rx thread each) */
    uint32_t max_batch;    /* largest n passed to the host-buffer entry points (staging)   */
    uint32_t max_bytes;    /* staging arena bytes for host-buffer entry points            */
    uint32_t flags;        /* RXG_CFG_*                                                    */
    uint32_t max_blocks;   /* rx grid cap in workgroups; 0 = one generation of resident
                              workgroups (occupancy).  Any value gives the same records.   */
    uint32_t zc_bytes;     /* rxg_rx_burst: bursts of up to this many staged bytes run
                              zero-copy (kernel reads pinned staging over PCIe); 0 = 64 MiB */
} rxg_config;

/* rxg_config.flags.  RXG_CFG_REPLAY_ON_DEVICE: rxg_rx_replay re-classifies every packet a
   handler's tcbs[] write affects with a GPU launch (the default answers small sets from the
   host index the device mirror is patched from; same records either way).
   RXG_CFG_STREAMS_OUTLIVE_WRITES: the write's order against table-reading launches on
   caller streams is taken when the write is pushed (an event recorded on the stream then)
   instead of by a marker after every launch, which on a caller stream cost ~4.5 us per
   launch.  The recording needs the stream to exist at the write, so in this
   mode a caller stream must be registered (rxg_stream_register) before its first
   table-reading launch (rxg_rx_burst_dev, rxg_rx_bursts_dev; else -EINVAL, nothing
   launched) and retired (rxg_stream_retire) before it is destroyed.  Without the flag a
   stream may be destroyed once synchronised. */
#define RXG_CFG_REPLAY_ON_DEVICE 0x1u
#define RXG_CFG_STREAMS_OUTLIVE_WRITES 0x2u

int rxg_abi_version(void);
/* "rxg src=<16 hex: sha256 of the product sources> rev=<git revision>[+dirty] built=<date>
   gfx950": which sources the library was built from (rxg.source_hash() recomputes src=). */
const char *rxg_build_info(void);
int rxg_init(const rxg_config *cfg, rxg_ctx **out);
/* 0, or -EIO when a latency-mode server kernel that missed its time limit is still resident
   after bounded retries of rxg_server_stop: the context and every buffer that kernel can
   reach are then left allocated (leaked), never freed under it; the handle is dead either way. */
int rxg_fini(rxg_ctx *ctx);
/* Block until all work queued on the context's stream is done. */
int rxg_sync(rxg_ctx *ctx);
/* The hipStream_t rxg launches on when a NULL stream is passed. */
void *rxg_stream(rxg_ctx *ctx);
/* Caller streams of a RXG_CFG_STREAMS_OUTLIVE_WRITES context (any context accepts them).
   register: `stream` may carry table-reading launches from now on.  retire: the context
   takes, now, the order its next table write needs against the stream's launches and forgets
   the stream; the caller may then destroy it.  The context's own stream needs neither.
   0, or -EINVAL for a NULL argument. */
int rxg_stream_register(rxg_ctx *ctx, void *stream);
int rxg_stream_retire(rxg_ctx *ctx, void *stream);

/* ------------------------------------------------------------------------- */
/* TCB mirror.  The reference mutates `tcbs[]` directly (tcp_tcb.c:21-22,     */
/* alloc_tcb :34-106, remove_tcb :175-186, tuple writes in socket_interface.c */
/* :80-83,:329-332 and tcp_states.c :25-27,:185-188).  A caller mirrors each   */
/* such write with one of these calls; they are applied to the device copy   */
/* before the next burst.                                                     */
/* ------------------------------------------------------------------------- */
typedef struct rxg_tcb_tuple {
    int32_t dport;       /* struct tcb::dport (host order, int)          tcp_tcb.h:17 */
    int32_t sport;       /* struct tcb::sport (host order, int)          tcp_tcb.h:18 */
    uint32_t ipv4_dst;   /* struct tcb::ipv4_dst, compared RAW to ip->dst_addr        */
    uint32_t ipv4_src;   /* struct tcb::ipv4_src, compared to ntohl(ip->src_addr)     */
    uint8_t state;       /* struct tcb::state (enum rxg_tcp_state)                    */
    uint8_t pad;
    uint16_t identifier; /* struct tcb::identifier (1..65535 cyclic)                  */
} rxg_tcb_tuple;

/* tcbs[idx] = tuple (a live slot).  idx >= current Ntcb grows Ntcb to idx+1; slots in
   between are NULL, as if allocated and removed. */
int rxg_tcb_upsert(rxg_ctx *ctx, int32_t idx, const rxg_tcb_tuple *t);
/* tcbs[idx] = NULL (remove_tcb).  Ntcb never shrinks (tcp_tcb.c:175-186). */
int rxg_tcb_remove(rxg_ctx *ctx, int32_t idx);
/* tcbs[idx]->state = state. */
int rxg_tcb_set_state(rxg_ctx *ctx, int32_t idx, uint8_t state);
/* Replace the whole table: tcbs[0..ntcb), live[i]==0 marks a NULL slot. */
int rxg_tcb_load(rxg_ctx *ctx, const rxg_tcb_tuple *tcbs, const uint8_t *live, int32_t ntcb);
/* Push pending mirror changes to the device (done implicitly by every burst).  Each write
   changes O(1) device words (a bucket slot, a listener entry), applied by one small kernel
   on the context's stream after every launch that still reads the old table, whatever its
   stream; a burst on another stream waits for them on the device, not on the host.  Only
   rxg_tcb_load and growth past load 1/2 rebuild (and upload) the whole table (see
   RXG_CFG_STREAMS_OUTLIVE_WRITES for bursts on caller streams). */
int rxg_tcb_sync(rxg_ctx *ctx);
/* Current Ntcb of the mirror. */
int32_t rxg_tcb_count(rxg_ctx *ctx);

/* Flow-affinity sharding (SURVEY.md §8(e)'s optional mode): one rx queue per
   GPU, the NIC steering each TCP segment to a queue by its RSS hash (Toeplitz over src ip,
   dst ip, src port, dst port with the default 40-byte Microsoft key, then a redirection table
   of RXG_RSS_RETA_SIZE entries filled round-robin, DPDK's default).  The context of queue
   `part` of `nparts` keeps in its device table only the tuples that hash to it (1/nparts of
   the keys); the listener map, liveness and the lowest NULL slot stay whole, so findtcb's
   pass 2 (tcp_tcb.c:158-170) answers as against the whole table.  Every context still gets
   every tcbs[] write (rxg_tcb_*).  A frame classified by the context of another queue
   finds no exact TCB: steer with the NIC or with rxg_flow_part_of.  nparts = 1: the whole
   table (the default).  Takes effect at the next sync (a table rebuild). */
#define RXG_RSS_RETA_SIZE 128
int rxg_flow_partition(rxg_ctx *ctx, uint32_t part, uint32_t nparts);
/* The context's partition (1 of 1 when not partitioned).  A group (rxg_group_*) cuts
   contiguous shards, so rxg_group_rx_burst refuses partitioned members (-EINVAL). */
int rxg_flow_partition_get(rxg_ctx *ctx, uint32_t *part, uint32_t *nparts);
/* The queue (0 .. nparts-1) an IPv4/TCP frame belongs to (frame bytes 26..37, read as the
   kernel reads them: bytes at or past len are zero); 0 for other frames, which no context
   looks up.  -EINVAL for frame NULL with len > 0 or nparts outside 1..RXG_RSS_RETA_SIZE. */
int rxg_flow_part_of(const uint8_t *frame, uint32_t len, uint32_t nparts);
/* The Toeplitz RSS hash of 12 wire bytes (src ip | dst ip | src port | dst port). */
uint32_t rxg_rss_hash(const uint8_t tuple12[12]);
/* Distinct tuples in the context's device table (after the last sync); -EINVAL for NULL. */
int64_t rxg_tcb_keys(rxg_ctx *ctx);

/* Writes from other threads.  The calls above belong to the rx thread (the one running
   bursts and rxg_rx_replay, whose tcpswitch handlers write tcbs[] on the reference's rx
   lcore).  The reference's socket API writes tcbs[] from the application lcore, unlocked
   against the rx loop (alloc_tcb tcp_tcb.c:34-106, socket_bind socket_interface.c:80-83,
   socket_connect :329-332); its mirror calls go through rxg_tcb_post instead: a lock-free
   multi-producer queue the rx thread drains, in claim order, at the start of the next
   burst (rxg_rx_burst, rxg_rx_burst_dev, rxg_ether_in) or rxg_tcb_sync / rxg_tcb_drain,
   so a burst never sees a half-applied write.  Not drained during rxg_rx_replay. */
enum rxg_tcb_op_kind { RXG_TCB_OP_UPSERT = 1, RXG_TCB_OP_REMOVE = 2, RXG_TCB_OP_SET_STATE = 3 };
typedef struct rxg_tcb_op {
    uint32_t kind;        /* enum rxg_tcb_op_kind                                   */
    int32_t idx;          /* tcbs[] index                                           */
    rxg_tcb_tuple tuple;  /* RXG_TCB_OP_UPSERT                                      */
    uint8_t state;        /* RXG_TCB_OP_SET_STATE                                   */
    uint8_t pad[3];
} rxg_tcb_op;
#define RXG_TCB_QUEUE_CAP 65536u
/* Any thread.  -EAGAIN when RXG_TCB_QUEUE_CAP posts are waiting (nothing queued then). */
int rxg_tcb_post(rxg_ctx *ctx, const rxg_tcb_op *op);
/* rx thread: apply every posted write now.  Returns how many were applied, or the first
   failing write's negative errno (the later ones are still applied). */
int rxg_tcb_drain(rxg_ctx *ctx);

/* ARP mirror (optional).  The reference keeps an IP -> MAC list that ip_in walks twice per
   packet (print_arp_table + get_mac, ip.c:26-32, arp.c:215-280).  Once a caller mirrors
   every add_mac (arp.c:282-317) with rxg_arp_learned, bursts flag each TCP packet whose
   source is unknown (RXG_F_ARP_LEARN) and rxg_rx_replay calls add_mac for the first such
   packet per address without walking the list: same final list, same order. */
int rxg_arp_load(rxg_ctx *ctx, const uint32_t *ipv4_host, uint32_t n);
int rxg_arp_learned(rxg_ctx *ctx, uint32_t ipv4_host);
int32_t rxg_arp_count(rxg_ctx *ctx);
/* Stop mirroring (RXG_F_ARP_LEARN is no longer computed; replay walks get_mac again). */
int rxg_arp_disable(rxg_ctx *ctx);

/* ------------------------------------------------------------------------- */
/* Receive burst: parse + checksum + classify.  Pure: no frees, no side       */
/* effects, counters only.                                                    */
/* ------------------------------------------------------------------------- */

/* Device-resident batch.  Frame i occupies bytes [frames + 64*off64[i],
   + len[i]); the bytes up to the next 64-byte boundary must be readable
   (their contents are ignored), and so must the first 64 bytes at `frames`
   (loads for chunks outside a frame are redirected there, then discarded).
   len[i] = rte_pktmbuf_data_len(m).  Alignment (else -EINVAL): frames 16 bytes, off64 4,
   len 2, out 8 (RXG_REC8) or 16 bytes. */
typedef struct rxg_dev_batch {
    const void *frames;     /* dev */
    const uint32_t *off64;  /* dev, n entries, in 64-byte units */
    const uint16_t *len;    /* dev, n entries */
    uint32_t n;
    uint32_t rec_kind;      /* RXG_REC8, RXG_REC16 or RXG_REC48 */
    void *out;              /* dev, n records of rec_kind bytes */
} rxg_dev_batch;

/* Replaces the per-packet loop over ether_in() (main.c:396-399) for a batch already
   resident in HBM.  Asynchronous on `stream`. */
int rxg_rx_burst_dev(rxg_ctx *ctx, const rxg_dev_batch *b, void *stream);

/* Several bursts of one frame pool in one launch (e.g. the bursts of several rx queues, or a
   ring of bursts): burst j's frame i is at frames + 64*bursts[j].off64[i] (same readability
   rules as rxg_dev_batch), its record at bursts[j].out + i * rec_kind.  Every burst is
   classified against the mirror as it stands at the call, exactly as k rxg_rx_burst_dev
   calls with no mirror writes between them; one launch (per 32 bursts) instead of k, so the
   launch ramp is paid once.  The bursts are then replayed in order, one rxg_rx_replay call
   each (a replay sees the tcbs[] writes of the earlier bursts' replays), and
   rxg_payload_gather_dev gathers the burst to be replayed next.  A burst with n == 0 may carry
   NULL pointers: it is skipped before any pointer is checked or read, and a call whose bursts
   are all empty launches nothing and returns 0.  Asynchronous on `stream`. */
typedef struct rxg_dev_burst {
    const uint32_t *off64;  /* dev, n entries, in 64-byte units of the frame pool */
    const uint16_t *len;    /* dev, n entries */
    uint32_t n;
    uint32_t pad;
    void *out;              /* dev, n records */
} rxg_dev_burst;
int rxg_rx_bursts_dev(rxg_ctx *ctx, const void *frames, const rxg_dev_burst *bursts, uint32_t k,
                      uint32_t rec_kind, void *stream);

/* Fixed-stride bursts: frame i of a burst occupies bytes [frames + 64 * (slot0 + i * stride64),
   + len[i]), with the readability rules of rxg_dev_batch.  For frame pools of fixed-size
   elements filled in ring order -- a DPDK mempool's elements are fixed-size (MBUF_SIZE,
   main.c:94-95), and a receive ring whose buffers are such elements posted in order, or this
   library's own host-burst staging, places frame i at a fixed stride -- the kernel then reads
   no per-frame offset list: 4 bytes less per frame of descriptor traffic (of 14 per 64-byte
   frame with 8-byte records).  Same records, counters, replay and payload gather as
   rxg_rx_bursts_dev with off64[i] = slot0 + i * stride64 (slot0 + (n-1) * stride64 must fit
   32 bits, else -EINVAL).  Asynchronous on `stream`. */
typedef struct rxg_dev_strided_burst {
    const uint16_t *len;    /* dev, n entries */
    uint32_t n;
    uint32_t slot0;         /* 64-byte slot of the burst's frame 0 in the pool */
    void *out;              /* dev, n records */
} rxg_dev_strided_burst;
int rxg_rx_bursts_strided_dev(rxg_ctx *ctx, const void *frames, uint32_t stride64,
                              const rxg_dev_strided_burst *bursts, uint32_t k, uint32_t rec_kind, void *stream);

/* DPDK-compatible host packet view: frame = (char*)buf_addr + data_off, data_len bytes
   (struct rte_mbuf fields of the same names). */
typedef struct rxg_pkt_view {
    const void *buf_addr;
    uint16_t data_off;
    uint16_t data_len;
    uint32_t pad;
} rxg_pkt_view;

/* Host-buffer burst: packs the frames into pinned staging, H2D, kernel, D2H into
   `out_host` (n records of rec_kind bytes).  Synchronous. */
int rxg_rx_burst(rxg_ctx *ctx, const rxg_pkt_view *pkts, uint32_t n, uint32_t rec_kind,
                 void *out_host);

/* Latency mode for the reference's own burst size (MAX_PKT_BURST = 32, main.c:116; the loop
   main.c:391-399 runs once per rte_eth_rx_burst).  A launched burst pays a kernel launch
   and a stream synchronisation (~20 us for 32 frames); the server is a persistent set of
   `blocks` workgroups of the same kernel body that polls a mailbox, so a burst costs the
   PCIe trips of its frames and records.  The host-burst staging (frames, descriptors)
   lives in device memory the host writes through the PCIe BAR (posted writes; the server
   reads HBM) when the device exposes its memory to the host (large BAR), else in coherent
   host memory (RXG_SRV_HOST_STAGING forces that); the mailbox the server polls is device
   memory too on such a device (RXG_SRV_HOST_MAILBOX keeps it in coherent host memory);
   the server's answers and the records of host bursts are written to host memory.
   While the server runs,
   rxg_rx_burst sends bursts of up to max_frames frames (max_bytes staged bytes) and of
   record kind rec_kind through it (packed into the server's own staging), and
   rxg_server_burst_dev serves device-visible batches.  Records, counters, replay and
   payload gather are those of the launched path.  A burst of up to 128 frames runs on the
   first workgroup (its four waves sharing one or two 64-frame slices of large frames); with
   `blocks` >= 3 a host
   burst of 129..64*blocks frames holding a frame over 64 bytes runs one 64-frame slice per
   workgroup, so `blocks` = 4 serves the reference's bursts and bursts of up to 256 large
   frames at the shortest latency.  The server exits by itself after idle_ms
   without a burst (and is relaunched by the next one), so it never outlives its process for
   long.  Calls from the context's rx thread only.  Returns 0 or a negative errno. */
typedef struct rxg_server_config {
    uint32_t rec_kind;    /* RXG_REC8 / RXG_REC16 / RXG_REC48 */
    uint32_t blocks;      /* workgroups (4 waves each); 0 = 1 */
    uint32_t max_frames;  /* largest burst served; 0 = 4096 */
    uint32_t max_bytes;   /* staging bytes for host bursts; 0 = max_frames * 2048 */
    uint32_t idle_ms;     /* exit after this long without a burst; 0 = 1000 */
    uint32_t flags;       /* RXG_SRV_*; 0 = mailbox and staging placed by the device */
} rxg_server_config;
#define RXG_SRV_HOST_STAGING 1u   /* staging in coherent host memory */
#define RXG_SRV_HOST_MAILBOX 2u   /* mailbox in coherent host memory */
int rxg_server_start(rxg_ctx *ctx, const rxg_server_config *cfg);
/* Stops the server and waits for its kernel to end; 0 if none runs. */
int rxg_server_stop(rxg_ctx *ctx);
/* 1 if a server is configured (running or idle-exited, relaunched on demand), else 0. */
int rxg_server_active(rxg_ctx *ctx);
/* Where the configured server's host-burst staging lives: RXG_SRV_DEVICE (device memory
   written through the BAR), RXG_SRV_HOST (coherent host memory), RXG_SRV_NONE (no server). */
#define RXG_SRV_NONE 0
#define RXG_SRV_HOST 1
#define RXG_SRV_DEVICE 2
int rxg_server_placement(rxg_ctx *ctx);
/* Classify a device-visible batch (HBM or mapped host memory) through the server:
   b->rec_kind must be the server's, b->n <= max_frames.  Synchronous: returns once the
   records are written at b->out.  -ENODEV without a server. */
int rxg_server_burst_dev(rxg_ctx *ctx, const rxg_dev_batch *b);

/* ------------------------------------------------------------------------- */
/* Transmit checksum generate: what ip_out computes (ip.c:97-118) for a batch  */
/* of frames whose Ethernet/IPv4/TCP headers the host has filled.  Writes      */
/* hdr_checksum (frame bytes 24-25) and tcp cksum (bytes 50-51) in place, both */
/* stored htons(calculate_checksum(..)) with the field zeroed while summing.   */
/* The TCP span is pseudo || frame[34 .. 14+total_length).                     */
/* ------------------------------------------------------------------------- */
typedef struct rxg_dev_tx_batch {
    void *frames;           /* dev, modified in place */
    const uint32_t *off64;  /* dev */
    const uint16_t *len;    /* dev */
    uint32_t n;
    uint32_t pad;
} rxg_dev_tx_batch;
int rxg_tx_cksum_dev(rxg_ctx *ctx, const rxg_dev_tx_batch *b, void *stream);

/* ------------------------------------------------------------------------- */
/* Transmit segment build: what sendtcpdata -> ip_out -> ether_out do per      */
/* segment (tcp_out.c:157-207, ip.c:86-118, etherout.c:87-99) for a batch of   */
/* segment descriptors, in one pass: the payload is read once from device      */
/* memory, each frame is written once with its Ethernet, IPv4 and TCP headers  */
/* and both checksums in place.                                                */
/*                                                                             */
/* Frame i is written at frames + 64 * off64[i] (off64 NULL: at frames + 64 *  */
/* (slot0 + i * stride64)) as 54 header bytes, data_len payload bytes and      */
/* zeros up to the next 64-byte boundary; nothing past that boundary is        */
/* written.  Header fields:                                                    */
/*   Ethernet  dst_mac, src_mac, 08 00                                         */
/*   IPv4      version_ihl 0x45, total_length htons(40 + data_len), packet_id  */
/*             ip_id as it stands (ip.c:106), ttl 127, proto 6, src_addr       */
/*             ipv4_dst as it stands, dst_addr htonl(ipv4_src), hdr_checksum   */
/*             as ip.c:107.  tos and fragment_offset are 0: the reference      */
/*             leaves them as whatever the fresh mbuf held, rxg defines them.  */
/*   TCP       src_port htons(dport), dst_port htons(sport), seq and ack       */
/*             htonl, data_off 0x50 (20 bytes, no options: what sendtcpdata,   */
/*             sendsyn, sendfin and send_reset build), tcp_flags, rx_win       */
/*             win_raw as it stands, urp 0, cksum as ip.c:109-118 over         */
/*             pseudo || header || payload (an odd last byte padded with 0).   */
/* The kernel reads only 16-byte aligned chunks that overlap [src_off,         */
/* src_off + data_len): the payload allocation is a multiple of 16 bytes.      */
/*                                                                             */
/* A segment with flow >= nflows, data_len > RXG_TX_MAX_DATA or src_off +      */
/* data_len > payload_bytes is skipped: len[i] = 0, nothing written to its     */
/* frame, stats[1] counts it; its flow index and offset are never followed.    */
/* -EINVAL: a NULL argument, frames not 64-byte aligned, payload not 16-, segs */
/* / flows / stats not 8-, off64 not 4-, len not 2-byte aligned, stride64 0 or */
/* slot0 + (n - 1) * stride64 over 2^32 - 1 in strided mode.  n == 0 does      */
/* nothing.                                                                    */
/* Asynchronous on `stream`, as rxg_tx_cksum_dev; the TCB and ARP mirrors are  */
/* neither read nor written.                                                   */
/* ------------------------------------------------------------------------- */
#define RXG_TX_MAX_DATA 65481u /* 54 + data_len fits the 16-bit frame length */
#define RXG_REF_SRC_MAC {0x6a, 0x9c, 0xba, 0xa0, 0x96, 0x24} /* etherout.c:94-99 */

typedef struct rxg_tx_flow { /* 32 bytes; the TCB fields sendtcpdata / ip_out read */
    uint16_t dport, sport;   /* as in rxg_tcb_tuple (host order)                          */
    uint32_t ipv4_dst;       /* raw network order, becomes ip src_addr (ip.c:97)          */
    uint32_t ipv4_src;       /* host order, htonl() of it becomes ip dst_addr (ip.c:99)   */
    uint8_t dst_mac[6];      /* what get_mac() returns for ipv4_src (etherout.c:176)      */
    uint8_t src_mac[6];
    uint8_t reserved[8];
} rxg_tx_flow;

typedef struct rxg_tx_seg { /* 32 bytes */
    uint64_t src_off;       /* byte offset of the payload in `payload`, any alignment     */
    uint32_t flow;          /* index into flows[]                                         */
    uint32_t seq, ack;      /* host order; stored htonl (tcp_out.c:176,187)               */
    uint16_t data_len;      /* 0 .. RXG_TX_MAX_DATA                                       */
    uint16_t win_raw;       /* stored without a byte swap, as tcp_out.c:190,310 do        */
    uint16_t ip_id;         /* stored without a byte swap, as ip.c:106 does               */
    uint8_t tcp_flags;
    uint8_t pad;
    uint32_t reserved;      /* ignored by rxg_tx_build_dev; rxg_tx_build_opt_dev: the segment's
                               option block, 0 = none, k = opts[k - 1]                       */
} rxg_tx_seg;

typedef struct rxg_dev_tx_build {
    const void *payload;      /* dev, 16-byte aligned base */
    uint64_t payload_bytes;
    const rxg_tx_flow *flows; /* dev */
    uint32_t nflows;
    uint32_t n;
    const rxg_tx_seg *segs;   /* dev, n entries */
    void *frames;             /* dev, 64-byte aligned */
    const uint32_t *off64;    /* dev, n entries; NULL = fixed stride */
    uint32_t slot0, stride64; /* used when off64 == NULL */
    uint16_t *len;            /* dev, n entries, written: 54 + data_len, 0 = skipped */
    uint64_t *stats;          /* dev, 2 words, added to: {built, skipped}; may be NULL */
} rxg_dev_tx_build;
int rxg_tx_build_dev(rxg_ctx *ctx, const rxg_dev_tx_build *b, void *stream);

/* Host-side planner (no context, no GPU): cuts each send into ceil(bytes / mss) segments
   (bytes 0: one segment without data).  Sequence numbers advance as tcp_out.c:176-185:
   + data_len per segment, + 1 for a segment carrying SYN, + 1 for one carrying FIN.  SYN goes
   on a send's first segment only, FIN and PSH on its last only, every other flag on all.
   ip_id counts up from ip_id0 (16-bit wrap).  Returns the number of segments written to out,
   -ENOSPC if cap is too small (nothing past cap is written), -EINVAL for mss 0 or over
   RXG_TX_MAX_DATA or a NULL sends / out.  next_seq_out[j] (may be NULL): the sequence number
   after send j. */
typedef struct rxg_tx_send {
    uint32_t flow;
    uint32_t next_seq, ack;
    uint64_t src_off;
    uint32_t bytes;
    uint8_t tcp_flags;
    uint8_t pad[3];
    uint16_t win_raw;
    uint16_t ip_id0;
} rxg_tx_send;
int64_t rxg_tx_plan(const rxg_tx_send *sends, uint32_t nsends, uint32_t mss, rxg_tx_seg *out, uint64_t cap,
                    uint32_t *next_seq_out);

/* ------------------------------------------------------------------------- */
/* Transmit segment build with TCP options: rxg_tx_build_dev for segments      */
/* that carry an option block between the TCP header and the payload, as the   */
/* reference's own ACK does (sendack -> sendtcpack, tcp_out.c:251-289: a       */
/* 40-byte TCP header) and as every data segment to a peer that negotiated     */
/* timestamps must.  The host fills a table of option blocks; a segment names  */
/* its block, the device needs no per-connection state for it.                 */
/*                                                                             */
/* In this call only, rxg_tx_seg.reserved selects the block: 0 = no options,   */
/* k in 1..nopts = opts[k - 1], O = opts[k - 1].len (0 otherwise).  Frame i    */
/* holds 54 header bytes, O option bytes (bytes[0..O) as they stand, at frame  */
/* bytes 54 .. 54 + O), data_len payload bytes and zeros up to the next        */
/* 64-byte boundary; nothing past that boundary is written.  len[i] = 54 + O + */
/* data_len.  Header fields are rxg_tx_build_dev's except                      */
/*   IPv4      total_length htons(40 + O + data_len)                           */
/*   TCP       data_off (5 + O / 4) << 4; cksum over pseudo || header ||       */
/*             options || payload, the pseudo-header's length htons(20 + O +   */
/*             data_len).                                                      */
/* The payload is read as by rxg_tx_build_dev (16-byte chunks overlapping      */
/* [src_off, src_off + data_len) only; data_len 0: none); of a block, its      */
/* 48 bytes.                                                                   */
/*                                                                             */
/* A segment is skipped under rxg_tx_build_dev's rules and when reserved >     */
/* nopts, when its block's len is over 40 or not a multiple of 4, or when      */
/* data_len > RXG_TX_MAX_DATA - O: len[i] = 0, nothing written to its frame,   */
/* stats[1] counts it; its flow index, source offset and block index are never */
/* followed, and a block is read only once reserved <= nopts is established.   */
/* -EINVAL: rxg_tx_build_dev's cases, opts not 16-byte aligned, opts NULL with */
/* nopts != 0.  n == 0 does nothing.  With every reserved == 0 the frames, len */
/* and stats are rxg_tx_build_dev's byte for byte.                             */
/* ------------------------------------------------------------------------- */

/* One TCP option block, 48 bytes, tables 16-byte aligned.  bytes[0..len) are stored at frame
   bytes 54 .. 54+len as they stand; len is 0, 4, .. 40.  The layout puts bytes[] at offset 6,
   so the three 16-byte chunks of the struct are the images of frame chunks 3, 4 and 5
   (frame bytes 48-95) from byte 54 on: the kernel loads them aligned, no shift.  Bytes of
   bytes[] at or past len, and the reserved fields, are ignored (not required to be zero). */
typedef struct rxg_tx_opt {
    uint8_t len;
    uint8_t reserved0[5];
    uint8_t bytes[40];
    uint8_t reserved1[2];
} rxg_tx_opt;

typedef struct rxg_dev_tx_build_opt {
    rxg_dev_tx_build b;     /* everything rxg_tx_build_dev takes, same rules           */
    const rxg_tx_opt *opts; /* dev, 16-byte aligned; may be NULL when nopts == 0       */
    uint32_t nopts;
    uint32_t pad;
} rxg_dev_tx_build_opt;
int rxg_tx_build_opt_dev(rxg_ctx *ctx, const rxg_dev_tx_build_opt *b, void *stream);

/* Host helpers for option blocks (no context, no GPU).
   rxg_tx_opt_set: n <= 40 bytes copied and padded with zero bytes to a multiple of 4 (zero is
   kind 0, end of option list: what the reference's memset(nop, 0, pad) writes, tcp_out.c:262),
   the rest of the struct zeroed.  Returns the padded length; -EINVAL for n > 40 or a NULL
   argument (bytes may be NULL when n == 0).
   rxg_tx_opt_timestamp: the 12 bytes 01 01 08 0A htonl(tsval) htonl(tsecr) (RFC 7323
   appendix A), the block a data segment carries.  Returns 12.
   rxg_tx_opt_ref_ack: the 20 bytes sendtcpack builds (tcp_out.c:255-262, structs tcp.h:37-54,
   all packed).  Each add_*_option prepends, so the last one called comes first in the frame:
     08 0A 18 19 03 00 00 00 00 00   timestamp, value 203032 and echo 0 stored without a byte
                                     swap (add_timestamp_option, tcp_out.c:66-74)
     02 04 05 14                     MSS htons(1300)
     03 03 07                        window scale 7
     00 00 00                        pad
   This is the order gcc's left-to-right evaluation of the operands of `+` in tcp_out.c:255
   gives; C leaves that order unspecified, and it has not been confirmed on a build of the
   reference.  The reference appends its pad after the data (rte_pktmbuf_append,
   tcp_out.c:261), rxg pads inside the block: for sendack, which sends no data, the two are
   the same bytes.  With this block, tcp_flags ACK, win_raw 12000 and data_len 0 the built
   frame is sendack's.  Returns 20. */
int rxg_tx_opt_set(rxg_tx_opt *o, const uint8_t *bytes, uint32_t n);
int rxg_tx_opt_timestamp(rxg_tx_opt *o, uint32_t tsval, uint32_t tsecr);
int rxg_tx_opt_ref_ack(rxg_tx_opt *o);

/* rxg_tx_plan for sends that carry options: every segment of send j gets reserved =
   send_opt[j] and at most mss - O payload bytes, O that block's len (the options come out of
   the MSS, RFC 6691).  send_opt NULL: rxg_tx_plan's output exactly.  -EINVAL additionally for
   send_opt[j] > nopts, a block length that is not 0..40 in steps of 4, mss <= O, or opts NULL
   where a block is named; nothing is written in these cases. */
int64_t rxg_tx_plan_opt(const rxg_tx_send *sends, uint32_t nsends, uint32_t mss, const uint32_t *send_opt,
                        const rxg_tx_opt *opts, uint32_t nopts, rxg_tx_seg *out, uint64_t cap,
                        uint32_t *next_seq_out);

/* The number of segments rxg_tx_plan_opt would write for these sends (send_opt NULL:
   rxg_tx_plan), with its -EINVAL cases (those about out and cap apart), writing nothing: the
   `n` of the build launch that follows rxg_tx_plan_dev, known to the caller who made the
   sends without a device-to-host wait.  Host, no context, no GPU. */
int64_t rxg_tx_plan_count(const rxg_tx_send *sends, uint32_t nsends, uint32_t mss, const uint32_t *send_opt,
                          const rxg_tx_opt *opts, uint32_t nopts);

/* ------------------------------------------------------------------------- */
/* Transmit segment plan on the device: rxg_tx_plan_opt's cut of sends into    */
/* segment descriptors, with the sends as the only thing that crosses to the   */
/* device: "sends in, frames out" with rxg_tx_build_dev / _opt_dev after it.   */
/*                                                                             */
/* Let O_j be the len of the block send j names (send_opt[j] = k: opts[k - 1]; */
/* 0 when k is 0 or send_opt is NULL) and m_j = mss - O_j.  Send j has nseg_j  */
/* = ceil(bytes / m_j) segments, one when bytes is 0.  first[j] is the sum of  */
/* nseg over the sends before j, first[nsends] = the total = count[0].         */
/* Segment q of send j is segs[first[j] + q]:                                  */
/*   src_off    send.src_off + q * m_j (64-bit)                                */
/*   flow, ack, win_raw   the send's                                           */
/*   data_len   m_j, the last segment bytes - (nseg_j - 1) * m_j               */
/*   seq        next_seq + q * m_j (mod 2^32), + 1 when q > 0 and the send     */
/*              carries SYN (tcp_out.c:176-185)                                */
/*   ip_id      (uint16_t)(ip_id0 + q)                                         */
/*   tcp_flags  SYN on segment 0 only, FIN and PSH on the last only, every     */
/*              other flag on all                                              */
/*   pad 0;  reserved = send_opt[j] (0 when send_opt is NULL)                  */
/* next_seq[j] = next_seq + bytes (mod 2^32), + 1 for SYN, + 1 for FIN.        */
/* When no send is refused and total <= cap this is rxg_tx_plan_opt's output   */
/* in all 32 bytes of every descriptor, and its next_seq_out; only then.       */
/*                                                                             */
/* Where the call differs from the host planner, which returns an error about  */
/* data this call has not read when it returns:                                */
/*   Refused sends.  A send is refused when send_opt[j] > nopts, when its      */
/*   block's len is over 40 or not a multiple of 4, or when mss <= O_j.  It    */
/*   gets no segments (first[j + 1] == first[j]), next_seq[j] is its next_seq  */
/*   unchanged and count[1] counts it.  A block is read only once send_opt[j]  */
/*   <= nopts is established.                                                  */
/*   Cap.  Segments with index >= cap are not written; count[0] and first[]    */
/*   still hold what the sends need (rxg_tx_reset_dev's cap / *count rule).    */
/* src_off is never followed, flow indices are not checked: the build does.    */
/* -EINVAL: a NULL ctx, b, sends, first or count; segs NULL with cap != 0;     */
/* sends, segs, first or count not 8-, opts not 16-, next_seq or send_opt not  */
/* 4-byte aligned; mss 0 or over RXG_TX_MAX_DATA; opts NULL with nopts != 0.   */
/* nsends == 0 writes count = {0, 0} and first[0] = 0, and nothing else.       */
/* Asynchronous on `stream`; a pure function of its arguments: it reads and    */
/* writes no mirror.  The context owns a small device buffer of per-tile sums  */
/* that all calls share: a call on another stream waits (on the device,        */
/* through an event) for the previous call on this context.                    */
/* ------------------------------------------------------------------------- */
typedef struct rxg_dev_tx_plan {
    const rxg_tx_send *sends;  /* dev, 8-byte aligned, nsends entries (40 bytes each)            */
    uint32_t nsends, mss;
    const uint32_t *send_opt;  /* dev, nsends entries, or NULL: no send carries a block          */
    const rxg_tx_opt *opts;    /* dev, 16-byte aligned; may be NULL when nopts == 0              */
    uint32_t nopts, pad;
    rxg_tx_seg *segs;          /* dev, 8-byte aligned, WRITTEN: segments 0 .. min(total, cap)    */
    uint64_t cap;              /* entries in segs                                                */
    uint64_t *first;           /* dev, nsends + 1 entries, WRITTEN: first[j] = index of send j's
                                  first segment, first[nsends] = total                           */
    uint32_t *next_seq;        /* dev, nsends entries, WRITTEN; may be NULL                      */
    uint64_t *count;           /* dev, 2 words, WRITTEN (not added to): {total, refused sends}   */
} rxg_dev_tx_plan;
int rxg_tx_plan_dev(rxg_ctx *ctx, const rxg_dev_tx_plan *b, void *stream);

/* ------------------------------------------------------------------------- */
/* Reset replies built on the device from a burst's records: what send_reset   */
/* -> ip_out -> ether_out do per offending packet (tcp_out.c:103-146,          */
/* ip.c:62-132, etherout.c:87-99).  A reset is built for every frame i whose   */
/* record has verdict RXG_V_RST_NOPCB or RXG_V_RST_LISTEN_NONSYN, in packet    */
/* order: reset k belongs to the k-th such frame, is written at out + 64 * k   */
/* and idx[k] = i.  Resets with k >= cap are not written; *count is set to the */
/* number the burst needs (as arena_used for the payload gather).              */
/*                                                                             */
/* A reset is one 64-byte line, a pure function of the first 64 bytes of the   */
/* offending frame "in" (bytes at and beyond len[i] read as zero, as the rx    */
/* kernel reads RXG_F_TRUNC frames; fixed offsets 14 / 34 whatever the IHL,    */
/* tcp_in.c:42-45), ip_id0 + k and src_mac:                                    */
/*   0-5    in[6..12), the offender's source MAC (see below)                   */
/*   6-11   src_mac;  12-13  08 00                                             */
/*   14     0x45; 15 and 20-21 zero (rxg's definition, as rxg_tx_build_dev)    */
/*   16-17  htons(40);  18-19  (uint16_t)(ip_id0 + k) as it stands (ip.c:106)  */
/*   22, 23 ttl 127, proto 6;  24-25  hdr_checksum as ip.c:107                 */
/*   26-29  in[30..34), the raw dst_addr;  30-33  in[26..30), the raw src_addr */
/*   34-35  in[36..38);  36-37  in[34..36)        (tcp_out.c:127-128)          */
/*   38-41  in[42..46), the offender's recv_ack;  42-45  0  (tcp_out.c:129-130)*/
/*   46, 47 0x50, RXG_TCP_FLAG_RST;  48-49  12000 unswapped (E0 2E)            */
/*   50-51  TCP checksum over pseudo || the 20 header bytes (ip.c:109-118)     */
/*   52-63  0                                                                  */
/* The destination MAC: ether_out takes it from get_mac(ntohl(dst_addr)), which */
/* after ip_in's learn (ip.c:30-32) is the offender's source MAC whenever the  */
/* address was learned from this frame or from one with the same MAC; that is  */
/* what rxg writes.  A stack that must honour an older ARP entry overwrites    */
/* bytes 0-5: no checksum covers them.                                         */
/*                                                                             */
/* frames / off64 / len / slot0 / stride64 follow rxg_dev_batch's readability  */
/* rules and rxg_dev_tx_build's strided form; recs are the burst's n records   */
/* as the burst wrote them.  The call is a pure function of its arguments: it  */
/* reads and writes no mirror and does not depend on the last burst of the     */
/* context.  Asynchronous on `stream`.  The context owns a small device buffer */
/* of per-slice counts that all calls share: a call on another stream waits    */
/* (on the device, through an event) for the previous call on this context.    */
/* -EINVAL: a NULL ctx, b, frames, len, recs, out, idx or count; a bad         */
/* rec_kind; frames not 16-byte or out not 64-byte aligned; idx or off64 not   */
/* 4-, len not 2-, count not 8-byte aligned, recs not 8- (RXG_REC8) or 16-byte */
/* aligned; stride64 0 or slot0 + (n - 1) * stride64 over 2^32 - 1 in strided  */
/* mode.  n == 0 writes *count = 0 and nothing else.                           */
/* A group's members are plain contexts for this call; groups have no          */
/* rxg_reset_take of their own.                                                */
/* ------------------------------------------------------------------------- */
typedef struct rxg_dev_tx_reset {
    const void *frames;       /* dev: the burst's frame pool (rxg_dev_batch readability rules)   */
    const uint32_t *off64;    /* dev, n entries; NULL = fixed stride (slot0 + i * stride64)      */
    const uint16_t *len;      /* dev, n entries                                                  */
    uint32_t slot0, stride64; /* used when off64 == NULL                                         */
    uint32_t n;
    uint32_t rec_kind;        /* RXG_REC8 / RXG_REC16 / RXG_REC48                                */
    const void *recs;         /* dev: the burst's n records, as the burst wrote them             */
    void *out;                /* dev, 64-byte aligned: reset k is written at out + 64 * k        */
    uint32_t *idx;            /* dev: idx[k] = packet index i of reset k                         */
    uint64_t cap;             /* slots in out / entries in idx                                   */
    uint64_t *count;          /* dev, 1 word, WRITTEN (not added to): resets the burst needs     */
    uint16_t ip_id0;          /* reset k carries packet_id (uint16_t)(ip_id0 + k), stored raw    */
    uint8_t src_mac[6];       /* Ethernet source (RXG_REF_SRC_MAC for the reference's)           */
} rxg_dev_tx_reset;
int rxg_tx_reset_dev(rxg_ctx *ctx, const rxg_dev_tx_reset *b, void *stream);

/* Host helper (no context, no GPU): gives a built reset another packet_id.  Stores ip_id as
   it stands at bytes 18-19 and recomputes hdr_checksum (bytes 24-25) over the 20 header bytes
   as ip.c:44-59,107 do. */
void rxg_reset_set_id(uint8_t *frame64, uint16_t ip_id);

/* Using the prebuilt resets during the replay.  rxg_reset_attach names host copies of a
   rxg_tx_reset_dev call's `out` and `idx` (nbuilt = min(count, cap) entries) for the burst
   the next rxg_rx_replay call on this context replays; the attachment ends when that replay
   returns, however it returns.  rxg_reset_take is called from the stack's send_reset while
   the replay runs a packet: if a reset was prebuilt for that packet it sets *frame_out to its
   64-byte slot (given ip_id with rxg_reset_set_id if it was built with another: the stack's
   count++ drifts whenever a handler sends something between two resets) and returns 1.
   It returns 0 -- the stack runs its own send_reset -- for a packet that became a reset only
   through re-classification, a reset past cap, a call outside a replay or with nothing
   attached.  A prebuilt reset that is no longer wanted (the frame was re-classified to
   RXG_V_DISPATCH) is passed over; a reset's bytes do not depend on the TCB mirror, so a
   prebuilt one never goes stale.  -EINVAL: ctx or frame_out NULL (attach: ctx NULL, or a NULL
   array with nbuilt != 0). */
int rxg_reset_attach(rxg_ctx *ctx, void *resets_host, const uint32_t *idx_host, uint64_t nbuilt);
int rxg_reset_take(rxg_ctx *ctx, uint16_t ip_id, void **frame_out);

/* ------------------------------------------------------------------------- */
/* Received TCP options parsed on the device from a burst's frames and         */
/* records: what a stack otherwise walks per packet on the rx core to echo a   */
/* timestamp (the tsecr of rxg_tx_opt_timestamp), to learn a SYN's MSS and     */
/* window scale, and to find a peer's SACK blocks.  The reference ignores      */
/* received options (its own ACK sends three, tcp_out.c:255-262); the rule     */
/* below is rxg's definition.                                                  */
/*                                                                             */
/* One rxg_rx_opt per frame of the burst, in packet order: record i belongs to */
/* frame i (dense, no compaction).                                             */
/*                                                                             */
/* Candidates.  Frame i is parsed when its record's verdict is RXG_V_DISPATCH, */
/* RXG_V_RST_NOPCB or RXG_V_RST_LISTEN_NONSYN (the frames the payload gather   */
/* takes: the replay may turn an RST into a DISPATCH).  Every other frame gets */
/* an all-zero record.                                                         */
/*                                                                             */
/* Option bytes.  The TCP header is at frame + 34 whatever the IHL             */
/* (tcp_in.c:42-45).  d = frame[46] >> 4.  d < 5: O = 0, RXG_O_BAD_DOFF is set */
/* and nothing is walked; otherwise O = 4 * d - 20 (0 .. 40).  The option      */
/* bytes are b[j] = frame[54 + j], j < O.  A byte at or beyond len[i] reads as */
/* zero (frame[46] too), as the rx kernel and the reset build read truncated   */
/* frames; RXG_O_CUT (54 + O > len[i]) says that it applied.                   */
/*                                                                             */
/* Walk.  p = 0.  While p < O, with k = b[p]:                                  */
/*   k == 0 (end of option list): stop.                                        */
/*   k == 1 (no-operation): p += 1, continue.                                  */
/*   p + 1 >= O (no length byte): RXG_O_MALFORMED, stop.                       */
/*   l = b[p + 1]; l < 2 or p + l > O: RXG_O_MALFORMED, stop.                  */
/*   (k, l) = (2, 4)   mss = b[p+2] << 8 | b[p+3], RXG_O_MSS                   */
/*            (3, 3)   wscale = b[p+2] as it stands (not clamped), _WSCALE     */
/*            (4, 2)   RXG_O_SACK_PERM                                         */
/*            (5, 10 / 18 / 26 / 34)  nsack = (l - 2) / 8, sack_off = 54 + p + */
/*                     2, RXG_O_SACK: the blocks (pairs of big-endian left and */
/*                     right edges) stay in the frame, at frame + sack_off     */
/*            (8, 10)  tsval = b[p+2..p+6), tsecr = b[p+6..p+10), both         */
/*                     big-endian on the wire, host order here, RXG_O_TS       */
/*            anything else: RXG_O_OTHER (another kind, or a known kind with   */
/*                     another length), the option is skipped                  */
/*   p += l.                                                                   */
/* A later occurrence of a kind replaces an earlier one.  What was found       */
/* before a RXG_O_MALFORMED stop is kept.  opt_len = O.  The record reports    */
/* what the header holds: whether an option is legal on this segment (an MSS   */
/* outside a SYN) is the stack's decision, tcp_flags is in the burst's record. */
/* ------------------------------------------------------------------------- */
enum rxg_rx_opt_flag {
    RXG_O_PARSED = 0x0001,    /* the frame was a candidate and was parsed                     */
    RXG_O_MSS = 0x0002,
    RXG_O_WSCALE = 0x0004,
    RXG_O_SACK_PERM = 0x0008,
    RXG_O_SACK = 0x0010,
    RXG_O_TS = 0x0020,
    RXG_O_OTHER = 0x0040,     /* at least one option was skipped                              */
    RXG_O_MALFORMED = 0x0080, /* the walk was ended by a bad length                           */
    RXG_O_CUT = 0x0100,       /* 54 + O > len[i]: option bytes past the frame read as zero    */
    RXG_O_BAD_DOFF = 0x0200   /* data_off >> 4 is below 5: O = 0, nothing walked              */
};

typedef struct rxg_rx_opt {   /* 16 bytes */
    uint32_t tsval, tsecr;    /* host order (big-endian on the wire); 0 without RXG_O_TS      */
    uint16_t mss;             /* host order; 0 without RXG_O_MSS                               */
    uint8_t  wscale;          /* the shift byte as it stands (not clamped); 0 without _WSCALE   */
    uint8_t  nsack;           /* 0..4 SACK blocks                                              */
    uint8_t  sack_off;        /* frame offset of the first block's left edge (56..86); 0 if none:
                                 the blocks stay in the frame, which the replay's caller holds */
    uint8_t  opt_len;         /* O                                                             */
    uint16_t flags;           /* RXG_O_*                                                       */
} rxg_rx_opt;

/* frames / off64 / len / slot0 / stride64 follow rxg_dev_batch's readability rules (only bytes
   up to the end of the 64-byte line holding a frame's last byte are read, plus the first 64
   bytes at `frames`) and rxg_dev_tx_reset's strided form; recs are the burst's n records as the
   burst wrote them.  The call is a pure function of its arguments: it reads and writes no
   mirror, does not depend on the last burst of the context and uses no buffer of the context.
   One launch, asynchronous on `stream`; rxg_config.max_blocks caps its grid, the output does
   not depend on the grid.
   -EINVAL: a NULL ctx, b, frames, len, recs or out; a bad rec_kind; frames or out not 16-byte
   aligned; off64 not 4-, len not 2-byte aligned, recs not 8- (RXG_REC8) or 16-byte aligned;
   stride64 0 or slot0 + (n - 1) * stride64 over 2^32 - 1 in strided mode.  n == 0 launches
   nothing and writes nothing.  A group's members are plain contexts for this call. */
typedef struct rxg_dev_rx_opts {
    const void *frames;       /* dev: the burst's frame pool                                     */
    const uint32_t *off64;    /* dev, n entries; NULL = fixed stride (slot0 + i * stride64)      */
    const uint16_t *len;      /* dev, n entries                                                  */
    uint32_t slot0, stride64; /* used when off64 == NULL                                         */
    uint32_t n;
    uint32_t rec_kind;        /* RXG_REC8 / RXG_REC16 / RXG_REC48                                */
    const void *recs;         /* dev: the burst's n records, as the burst wrote them             */
    rxg_rx_opt *out;          /* dev, 16-byte aligned, n records                                 */
} rxg_dev_rx_opts;
int rxg_rx_opts_dev(rxg_ctx *ctx, const rxg_dev_rx_opts *b, void *stream);

/* Host form of the rule (no context, no GPU): one frame taken as a TCP segment -- the caller
   has the verdict -- parsed into *out (RXG_O_PARSED always set).  Reads frame[0 .. len) only.
   For frames that reach the stack outside a burst's option pass.  -EINVAL: out NULL, or frame
   NULL with len > 0. */
int rxg_rx_opt_parse(const uint8_t *frame, uint32_t len, rxg_rx_opt *out);

/* Using the parsed options during the replay.  rxg_rx_opts_attach names a host copy of a
   rxg_rx_opts_dev call's `out` (n records) for the burst the next rxg_rx_replay call on this
   context replays; the attachment ends when that replay returns, however it returns.
   rxg_rx_opt_current is called from a handler (tcpswitch, send_reset, ..) while the replay
   runs a packet: it sets *out = &opts_host[that packet's index] and returns 1 -- for a packet
   the replay re-classified too: options do not depend on the TCB mirror, so they never go
   stale.  It returns 0 outside a replay, with nothing attached, or when n differs from the
   replayed burst's.  -EINVAL: ctx or out NULL (attach: ctx NULL, or opts_host NULL with
   n != 0). */
int rxg_rx_opts_attach(rxg_ctx *ctx, const rxg_rx_opt *opts_host, uint32_t n);
int rxg_rx_opt_current(rxg_ctx *ctx, const rxg_rx_opt **out);

/* ------------------------------------------------------------------------- */
/* A burst summarised per flow from its records: what on_segment does per      */
/* dispatched frame (tcp_in.c:66-71: the max_seq_received update and           */
/* AdjustSendWindow(tcb, ack)) is a property of the flow, not of the packet.   */
/* max_seq_received is the unsigned 32-bit maximum of sent_seq (tcp_in.c:66 is */
/* a plain >, no serial-number arithmetic), and k calls AdjustSendWindow(tcb,  */
/* a_1..a_k) leave the send window as one call with the unsigned maximum of    */
/* the a_j does (tcp_windows.c:265 removes pairs with m_EndSeqNumber <=        */
/* AckValue; the early returns at :236 and :241 return only where that loop    */
/* would remove nothing).                                                      */
/*                                                                             */
/* Which frames count.  Frame i is counted when its record's verdict is        */
/* RXG_V_DISPATCH, 0 <= tcb_idx < ntcb and, with RXG_FS_TCP_OK_ONLY, its       */
/* record carries RXG_F_TCP_OK.  A DISPATCH record with tcb_idx outside        */
/* [0, ntcb) is never followed: count[1] counts it.  A DISPATCH frame left out */
/* by the checksum flag alone is counted in count[2].  Every other verdict is  */
/* ignored.                                                                    */
/*                                                                             */
/* Where each field comes from.  datalen, tcp_flags, state and tcb_idx come    */
/* from the record (rxg_rec8 decoded as rxg_rec8_expand does: state 7 becomes  */
/* RXG_STATE_NONE).  seq and ack are, for RXG_REC8 and RXG_REC16, big-endian   */
/* frame[38..42) and frame[42..46) with bytes at or beyond len[i] read as zero */
/* (as the rx kernel and the reset build read truncated frames); for RXG_REC48 */
/* they are the record's seq and ack and no frame byte is read: frames, off64  */
/* and len may then be NULL.                                                   */
/*                                                                             */
/* Output.  One rxg_flow_sum per TCB with at least one counted frame, in       */
/* ascending tcb_idx: out[k] is the k-th such TCB.  Entries with k >= cap are  */
/* not written.  count is 3 words, WRITTEN (not added to): count[0] the number */
/* of flows the burst touches whatever cap is (rxg_tx_reset_dev's cap / *count */
/* rule), count[1] and count[2] as above.  The output is a pure function of    */
/* the arguments: never of the grid, the stream, the mirror or an earlier call.*/
/* ------------------------------------------------------------------------- */
typedef struct rxg_flow_sum {   /* 40 bytes, arrays 8-byte aligned */
    int32_t  tcb_idx;
    uint32_t frames;        /* counted frames of this TCB                                    */
    uint32_t max_seq;       /* unsigned max of ntohl(sent_seq)   (tcp_in.c:66-67)             */
    uint32_t max_ack;       /* unsigned max of ntohl(recv_ack)   (one AdjustSendWindow call)  */
    uint32_t first_idx;     /* lowest and highest packet index among them                    */
    uint32_t last_idx;
    uint32_t data_frames;   /* frames with datalen > 0                                       */
    uint8_t  tcp_flags_or;  /* OR of their tcp_flags                                         */
    uint8_t  state;         /* the state field of frame first_idx's record                   */
    uint16_t reserved;      /* 0                                                             */
    uint64_t data_bytes;    /* sum of datalen over frames with datalen > 0                   */
} rxg_flow_sum;
#define RXG_FS_TCP_OK_ONLY 0x1u  /* leave out frames without RXG_F_TCP_OK (RXG_OPS_VERIFY_TCP_CKSUM stacks) */
#define RXG_FS_MAX_NTCB (1u << 24) /* rxg_rec8's index width */

/* frames / off64 / len / slot0 / stride64 follow rxg_dev_rx_opts' rules and strided form (of a
   counted frame only the 16 bytes at 32..47 are read, and only when len[i] > 38); recs are the
   burst's n records as the burst wrote them.  Asynchronous on `stream`: four launches (the
   accumulation, the per-tile counts of the touched bitmap, their scan, the expansion), no
   workgroup waits on another; rxg_config.max_blocks caps the grids.  The context owns a dense
   accumulator of ntcb entries and a touched bitmap that all calls share and every call leaves
   all zero; they grow on demand.  One call at a time uses them: a call on another stream waits
   (on the device, through an event) for the previous call on this context.
   n == 0 writes count = {0, 0, 0} and nothing else.
   -EINVAL: a NULL ctx, b, recs or count; out NULL with cap != 0; frames or len NULL unless
   rec_kind is RXG_REC48; a bad rec_kind; ntcb 0 or over RXG_FS_MAX_NTCB; unknown flag bits;
   frames not 16-, out or count not 8-, off64 not 4-, len not 2-byte aligned, recs not 8-
   (RXG_REC8) or 16-byte aligned; where frames are read, stride64 0 or slot0 + (n - 1) *
   stride64 over 2^32 - 1 in strided mode.  -ENOMEM: the accumulator cannot be allocated;
   nothing is launched then.  A group's members are plain contexts for this call. */
typedef struct rxg_dev_flow_sums {
    const void *frames;       /* dev: the burst's frame pool; may be NULL for RXG_REC48          */
    const uint32_t *off64;    /* dev, n entries; NULL = fixed stride (slot0 + i * stride64)      */
    const uint16_t *len;      /* dev, n entries; may be NULL for RXG_REC48                       */
    uint32_t slot0, stride64; /* used when off64 == NULL                                         */
    uint32_t n;
    uint32_t rec_kind;        /* RXG_REC8 / RXG_REC16 / RXG_REC48                                */
    const void *recs;         /* dev: the burst's n records, as the burst wrote them             */
    uint32_t ntcb;            /* 1 .. RXG_FS_MAX_NTCB: TCB indices at or past it are not followed */
    uint32_t flags;           /* RXG_FS_*                                                        */
    rxg_flow_sum *out;        /* dev, 8-byte aligned, cap entries                                */
    uint64_t cap;
    uint64_t *count;          /* dev, 3 words, WRITTEN: flows, DISPATCH out of range, left out   */
} rxg_dev_flow_sums;
int rxg_flow_sums_dev(rxg_ctx *ctx, const rxg_dev_flow_sums *b, void *stream);

/* Host form of the rule (no context, no GPU), for host-buffer bursts (rxg_rx_burst): frame i
   is frames[i][0 .. len[i]); frames and len may be NULL for RXG_REC48.  Returns 0; -EINVAL: recs
   or count NULL (n != 0 for recs), out NULL with cap != 0, frames or len NULL unless RXG_REC48
   (n != 0), a bad rec_kind, ntcb 0 or over RXG_FS_MAX_NTCB, unknown flag bits; -ENOMEM. */
int rxg_flow_sums_host(const void *recs, uint32_t rec_kind, void *const *frames, const uint16_t *len,
                       uint32_t n, uint32_t ntcb, uint32_t flags, rxg_flow_sum *out, uint64_t cap,
                       uint64_t count[3]);

/* Using the summaries during the replay.  rxg_flow_sums_attach names a host copy of a call's
   `out` (m = min(count[0], cap) entries, ascending tcb_idx) for the burst the next
   rxg_rx_replay call on this context replays; the attachment ends when that replay returns,
   however it returns.  rxg_flow_sum_current is called from a handler (on_segment, tcpswitch)
   while the replay runs a packet.  It returns 1, with *out the flow's summary and *pkt_idx the
   packet's index, when the packet's record as the burst wrote it is a DISPATCH whose TCB is
   in the attached list with first_idx <= index <= last_idx, and the replay did not replace
   that record by re-classification.  It returns 0 otherwise: outside a replay, with nothing
   attached, for a re-classified packet, or for a flow past cap.  (A frame a summary made with
   RXG_FS_TCP_OK_ONLY left out reaches no handler under RXG_OPS_VERIFY_TCP_CKSUM.)
   -EINVAL: ctx, out or pkt_idx NULL (attach: ctx NULL, a NULL array with m != 0, or entries
   not strictly ascending in tcb_idx). */
int rxg_flow_sums_attach(rxg_ctx *ctx, const rxg_flow_sum *sums_host, uint64_t m);
int rxg_flow_sum_current(rxg_ctx *ctx, const rxg_flow_sum **out, uint32_t *pkt_idx);

/* ------------------------------------------------------------------------- */
/* A burst's data segments grouped by flow and cut into in-order trains: which */
/* segments of one connection follow each other in sequence space, and how far */
/* they take that connection's stream (ptcb->ack after the burst,              */
/* tcp_windows.c:355, the value AdjustPair returns).                           */
/*                                                                             */
/* Which frames are segments.  Frame i is a segment when its record's verdict  */
/* is RXG_V_DISPATCH, 0 <= tcb_idx < ntcb, with RXG_FT_TCP_OK_ONLY its record  */
/* carries RXG_F_TCP_OK, and 0 < datalen <= 65535 (what PushData's uint16_t    */
/* Length can express, tcp_windows.c:341).  Counts, exactly as in              */
/* rxg_flow_sums_dev: a DISPATCH record whose tcb_idx is outside [0, ntcb) is  */
/* never followed and is counted in count[2]; a DISPATCH frame left out by the */
/* checksum flag alone is counted in count[3]; everything else is ignored.     */
/*                                                                             */
/* Where the fields come from.  tcb_idx, datalen and tcp_flags come from the   */
/* record (rxg_rec8 decoded as rxg_rec8_expand does).  seq is, for RXG_REC8    */
/* and RXG_REC16, big-endian frame[38..42) with bytes at or beyond len[i] read */
/* as zero; for RXG_REC48 it is the record's seq and no frame byte is read:    */
/* frames, off64 and len may then be NULL (the flow summary's rule).           */
/*                                                                             */
/* Order.  order[0..S) holds the packet indices of the S segments sorted by    */
/* (tcb_idx ascending, packet index ascending): a stable grouping, within a    */
/* flow the segments stand in the order they arrived.                          */
/*                                                                             */
/* Trains.  Walk a flow's segments in that order.  Segment b continues segment */
/* a, the one before it in the same flow, when seq_b == (uint32_t)(seq_a +     */
/* datalen_a), a does not carry FIN, and neither a nor b is a wrapping         */
/* segment.  A segment wraps when (uint64_t)seq + datalen >= 2^32: the         */
/* reference's duplicate test `cur > seq + Length` (tcp_windows.c:350)         */
/* compares a wrapped sum and drops such a segment, so a wrapping segment is   */
/* always a train of its own and is flagged.  A train is a maximal run of      */
/* continuing segments; trains are written in the order of `order`: train k's  */
/* segments are order[first .. first + nseg).                                  */
/*                                                                             */
/* HEAD.  cur_seq is an optional array of ntcb words, the stack's              */
/* ReceiveWindow.CurrentSequenceNumber per TCB; with NULL no train is HEAD.    */
/* For a flow whose window holds no pairs and whose CurrentSequenceNumber is   */
/* cur_seq[tcb_idx], a HEAD train's segments fed to the reference's PushData   */
/* one at a time are none refused, each becomes one socket-ring message,       */
/* whole; the messages concatenated are the train's payload bytes; ptcb->ack   */
/* ends as next_ack and CurrentSequenceNumber as (uint32_t)(seq + bytes).  The */
/* != 0 condition is GetData's assert (tcp_windows.c:151), as in               */
/* rxg_payload_take.  Two deliberate cuts, both conservative: only a flow's    */
/* first train can be HEAD, and a FIN ends its train although the reference's  */
/* CurrentSequenceNumber does not count the FIN.  For every train that is not  */
/* HEAD the stack runs its own PushData: the cuts cost speed, never            */
/* correctness.                                                                */
/*                                                                             */
/* Outputs and caps.  order has cap_seg entries, trains cap_trains; entries at */
/* or past a cap are not written.  count is 4 words, WRITTEN (not added to):   */
/* segments S, trains T, DISPATCH out of range, left out; count[0] and         */
/* count[1] are what the burst needs whatever the caps are (rxg_tx_reset_dev's */
/* cap / *count rule).  A train is written whole or not at all, and its first  */
/* and nseg are correct even if order was capped short of them.  n == 0 writes */
/* count = {0, 0, 0, 0} and nothing else.  The output is a pure function of    */
/* the arguments: never of the grid, the stream, the mirror or an earlier call.*/
/* ------------------------------------------------------------------------- */
typedef struct rxg_flow_train {   /* 32 bytes, arrays 8-byte aligned */
    int32_t  tcb_idx;
    uint32_t first;      /* its segments are order[first .. first + nseg)                    */
    uint32_t nseg;
    uint32_t seq;        /* ntohl(sent_seq) of its first segment                             */
    uint64_t bytes;      /* sum of datalen over its segments                                 */
    uint32_t next_ack;   /* (uint32_t)(seq + bytes) + (FIN ? 1 : 0): what AdjustPair returns */
                         /* after the train has been delivered (tcp_windows.c:104-109)       */
    uint32_t flags;      /* RXG_FTR_*                                                        */
} rxg_flow_train;
#define RXG_FTR_HEAD       0x01u /* the flow's first train, cur_seq given, cur_seq[tcb_idx] != 0 and == seq, not WRAP */
#define RXG_FTR_FIN        0x02u /* its last segment carries FIN                               */
#define RXG_FTR_WRAP       0x04u /* a single wrapping segment                                  */
#define RXG_FTR_FLOW_FIRST 0x08u /* first / last train of its flow in this burst               */
#define RXG_FTR_FLOW_LAST  0x10u
#define RXG_FT_TCP_OK_ONLY 0x1u  /* leave out frames without RXG_F_TCP_OK (RXG_OPS_VERIFY_TCP_CKSUM stacks) */

/* frames / off64 / len / slot0 / stride64 / recs / ntcb follow rxg_dev_flow_sums' rules (of a
   segment only the 16 bytes at 32..47 are read, and only when len[i] > 38).  Asynchronous on
   `stream`: a select (slice counts, their scan, a compaction into (tcb_idx, packet index)
   pairs), a least-significant-digit radix sort of the pairs on tcb_idx (8 bits a pass; 1 pass
   up to 256 TCBs, 2 up to 65 536, 3 above; each a per-tile digit count, a scan and a scatter
   without atomics) and a cut (per-tile train starts, their scan, the start list, one lane per
   train); no workgroup waits on another, and rxg_config.max_blocks caps the grids.  The
   context owns the scratch (about 30 bytes per frame), grown on demand; one call at a time uses it:
   a call on another stream waits (on the device, through an event) for the previous call on
   this context.
   -EINVAL: a NULL ctx, b, recs or count; order NULL with cap_seg != 0; trains NULL with
   cap_trains != 0; frames or len NULL unless rec_kind is RXG_REC48; a bad rec_kind; ntcb 0 or
   over RXG_FS_MAX_NTCB; unknown flag bits; frames not 16-, trains or count not 8-, cur_seq,
   order or off64 not 4-, len not 2-byte aligned, recs not 8- (RXG_REC8) or 16-byte aligned;
   where frames are read, stride64 0 or slot0 + (n - 1) * stride64 over 2^32 - 1 in strided
   mode.  -ENOMEM: the scratch cannot be allocated; nothing is launched then.  A group's
   members are plain contexts for this call. */
typedef struct rxg_dev_flow_trains {
    const void *frames;       /* dev: the burst's frame pool; may be NULL for RXG_REC48          */
    const uint32_t *off64;    /* dev, n entries; NULL = fixed stride (slot0 + i * stride64)      */
    const uint16_t *len;      /* dev, n entries; may be NULL for RXG_REC48                       */
    uint32_t slot0, stride64; /* used when off64 == NULL                                         */
    uint32_t n;
    uint32_t rec_kind;        /* RXG_REC8 / RXG_REC16 / RXG_REC48                                */
    const void *recs;         /* dev: the burst's n records, as the burst wrote them             */
    uint32_t ntcb;            /* 1 .. RXG_FS_MAX_NTCB: TCB indices at or past it are not followed */
    uint32_t flags;           /* RXG_FT_*                                                        */
    const uint32_t *cur_seq;  /* dev, ntcb words, 4-byte aligned; NULL: no train is HEAD         */
    uint32_t *order;          /* dev, 4-byte aligned, cap_seg entries                            */
    uint64_t cap_seg;
    rxg_flow_train *trains;   /* dev, 8-byte aligned, cap_trains entries                         */
    uint64_t cap_trains;
    uint64_t *count;          /* dev, 4 words, WRITTEN: segments, trains, out of range, left out */
} rxg_dev_flow_trains;
int rxg_flow_trains_dev(rxg_ctx *ctx, const rxg_dev_flow_trains *b, void *stream);

/* Host form of the rule (no context, no GPU), for host-buffer bursts (rxg_rx_burst): frame i
   is frames[i][0 .. len[i]); frames and len may be NULL for RXG_REC48; cur_seq is ntcb words
   of host memory or NULL.  Returns 0; -EINVAL: recs or count NULL (n != 0 for recs), order
   NULL with cap_seg != 0, trains NULL with cap_trains != 0, frames or len NULL unless
   RXG_REC48 (n != 0), a bad rec_kind, ntcb 0 or over RXG_FS_MAX_NTCB, unknown flag bits;
   -ENOMEM. */
int rxg_flow_trains_host(const void *recs, uint32_t rec_kind, void *const *frames, const uint16_t *len,
                         uint32_t n, uint32_t ntcb, uint32_t flags, const uint32_t *cur_seq, uint32_t *order,
                         uint64_t cap_seg, rxg_flow_train *trains, uint64_t cap_trains, uint64_t count[4]);

/* Using the trains during the replay.  rxg_flow_trains_attach names host copies of a call's
   `order` (nseg = min(count[0], cap_seg) entries) and `trains` (ntrains = min(count[1],
   cap_trains) entries) for the burst the next rxg_rx_replay call on this context replays; the
   attachment ends when that replay returns, however it returns.  rxg_flow_train_current is
   called from a handler (PushData's call site) while the replay runs a packet.  It returns 1,
   with *out the packet's train and *pos its position in that train (order[first + *pos] is
   the packet), when the packet is a segment of an attached train that lies whole inside the
   attached order and the replay did not replace the packet's record by re-classification.
   It returns 0 otherwise: outside a replay, with nothing attached, for a re-classified
   packet, for a packet that is no segment, or for a segment or train past a cap.
   -EINVAL: ctx, out or pos NULL (attach: ctx NULL, a NULL array with a nonzero length, or
   trains that do not tile [0, nseg) in order: train k must start where train k - 1 ended,
   train 0 at 0, nseg >= 1 each, tcb_idx never descending; trains whose segments lie past
   nseg may follow). */
int rxg_flow_trains_attach(rxg_ctx *ctx, const uint32_t *order_host, uint64_t nseg,
                           const rxg_flow_train *trains_host, uint64_t ntrains);
int rxg_flow_train_current(rxg_ctx *ctx, const rxg_flow_train **out, uint32_t *pos);

/* ------------------------------------------------------------------------- */
/* A burst's payload gathered by train: each train's bytes contiguous in the   */
/* arena, in sequence order, with one message per segment (what                */
/* rxg_payload_take answers from) and one per train (what a stream reader      */
/* takes whole).  The inputs are a burst and the outputs of                    */
/* rxg_flow_trains_dev / rxg_flow_trains_host on it: order, trains, count.     */
/*                                                                             */
/* Which trains take part.  S' = min(count[0], cap_seg, n), T' = min(count[1], */
/* cap_trains, n) (a burst of n frames has no more segments or trains than n); */
/* with S' == 0, T' is taken as 0.  Train k < T' takes part when               */
/* its segments lie whole inside order[0, S'): (uint64_t)first + nseg <= S'    */
/* (and bytes < 2^32, as every train the flow-train call writes has); with     */
/* RXG_TP_HEAD_ONLY it must also carry RXG_FTR_HEAD.  A WRAP train takes part  */
/* like any other (rxg_payload_take refuses its segment at replay time).       */
/*                                                                             */
/* Placement.  The taking trains are placed in train order: train k's span     */
/* starts at train_off = the sum of (bytes + 15) & ~15 over the taking trains  */
/* before it, so every span starts 16-byte aligned.  *arena_used is that sum   */
/* over all taking trains, whatever arena_cap is.  A taking train is placed    */
/* when train_off + ((bytes + 15) & ~15) <= arena_cap; the trains that are not */
/* are a suffix of the taking trains, and nothing of them is gathered.         */
/*                                                                             */
/* Bytes.  Segment j of a placed train (packet i = order[first + j]) is a      */
/* candidate when i < n, its record's verdict is DISPATCH, RST_NOPCB or        */
/* RST_LISTEN_NONSYN, datalen > 0, RXG_F_TRUNC is clear, len[i] > 46, and with */
/* start = 34 + (frame[46] >> 4) * 4 (GetData's address, tcp_windows.c:164-166:*/
/* the IP header taken as 20 bytes) start + datalen <= len[i]: the rule of     */
/* rxg_payload_gather_dev.  Its place is rel = (uint32_t)(seq_i - seq_train),  */
/* seq_i read as rxg_flow_trains_dev reads it; a candidate must also lie       */
/* inside its train, rel + datalen <= bytes (always so for the trains the      */
/* flow-train call wrote for this burst).  A candidate's datalen payload bytes */
/* frame[start ..) are written at arena + train_off + rel.  A segment that is  */
/* no candidate is a hole: its bytes in the span are left untouched and its    */
/* train's message carries RXG_PM_HOLE.  The pad bytes of a placed train,      */
/* [train_off + bytes, train_off + ((bytes + 15) & ~15)), are written as zero. */
/* No other byte of the arena is written.                                      */
/*                                                                             */
/* msgs[i], one per FRAME of the burst (may be NULL): for a copied segment     */
/* {train_off + rel, datalen, RXG_PM_GATHERED | RXG_PM_REF_OVERSIZE where      */
/* datalen >= 1000}; arena_off is not 16-byte aligned.  Every other frame's    */
/* message is all zero.  tmsgs[k], one per TRAIN k < T' (may be NULL): for a   */
/* placed train {train_off, (uint32_t)bytes, RXG_PM_GATHERED | RXG_PM_HOLE if  */
/* it has a hole}; for a train that does not take part or is not placed, all   */
/* zero.  tmsgs[k] for k >= T' is not written.                                 */
/*                                                                             */
/* n == 0: *arena_used = 0 and nothing else.  S' == 0: *arena_used = 0, msgs   */
/* (if given) all zero, nothing else.  The output is a pure function of the    */
/* arguments: never of the grid, the stream or an earlier call.                */
/* ------------------------------------------------------------------------- */
#define RXG_TP_HEAD_ONLY 0x1u  /* only trains that carry RXG_FTR_HEAD take part */

struct rxg_payload_msg;        /* (defined with the payload hand-off below) */

/* frames / off64 / len / slot0 / stride64 / recs / rec_kind name the burst as rxg_dev_flow_trains
   does, but frames and len are required for every record kind (the payload is read from the
   frame).  Asynchronous on `stream`: msgs zeroed, then four launches -- the taking trains' padded
   sizes summed per tile of 256 trains, a one-workgroup scan of the tile sums (which writes
   *arena_used), the trains' offsets and tmsgs, and the copy: a workgroup per tile of 256
   consecutive entries of `order` finds its first segment's train by a search over
   trains[].first, the other segments' by marking the train starts inside the tile, and shares
   the tile's 16-byte destination chunks out over its lanes.  Nothing waits on another workgroup,
   no atomic decides a position (RXG_PM_HOLE is ORed into a train's flags), count is read on the
   device only, and rxg_config.max_blocks caps the grids.  Payloads are read with 16-byte loads
   inside the 64-byte slots a frame's len occupies.  The context owns the scratch (8 bytes per
   train), grown on demand; one call at a time uses it, as for rxg_flow_trains_dev.
   When msgs is not NULL the call registers the burst for rxg_payload_take exactly as
   rxg_payload_gather_dev does (msgs and arena_used must stay valid until the burst's replay is
   done; one such call or gather is in flight per context); arena_used is never UINT64_MAX.
   -EINVAL: a NULL ctx, p, frames, len, recs, order (cap_seg != 0), trains (cap_trains != 0),
   count, arena_used, or arena with arena_cap != 0; a bad rec_kind; unknown flag bits; frames or
   arena not 16-, msgs, tmsgs, trains, count or arena_used not 8-, order or off64 not 4-, len
   not 2-byte aligned, recs not 8- (RXG_REC8) or 16-byte aligned; stride64 0 or slot0 + (n - 1) *
   stride64 over 2^32 - 1 in strided mode.  -ENOMEM: the scratch cannot be allocated; nothing is
   launched then. */
typedef struct rxg_dev_train_payload {
    const void *frames;       /* dev: the burst's frame pool                                     */
    const uint32_t *off64;    /* dev, n entries; NULL = fixed stride (slot0 + i * stride64)      */
    const uint16_t *len;      /* dev, n entries                                                  */
    uint32_t slot0, stride64; /* used when off64 == NULL                                         */
    uint32_t n;
    uint32_t rec_kind;        /* RXG_REC8 / RXG_REC16 / RXG_REC48                                */
    const void *recs;         /* dev: the burst's n records                                      */
    const uint32_t *order;    /* dev: rxg_flow_trains_dev's order for this burst, cap_seg entries */
    uint64_t cap_seg;
    const rxg_flow_train *trains; /* dev: its trains, cap_trains entries                         */
    uint64_t cap_trains;
    const uint64_t *count;    /* dev: its 4 count words, read on the device                      */
    uint32_t flags;           /* RXG_TP_*                                                        */
    void *arena;             /* dev, 16-byte aligned, arena_cap bytes                           */
    uint64_t arena_cap;
    struct rxg_payload_msg *msgs;   /* dev, n entries, one per FRAME; may be NULL                */
    struct rxg_payload_msg *tmsgs;  /* dev, cap_trains entries, one per TRAIN; may be NULL       */
    uint64_t *arena_used;     /* dev, 1 word, WRITTEN                                            */
} rxg_dev_train_payload;
int rxg_train_payload_dev(rxg_ctx *ctx, const rxg_dev_train_payload *p, void *stream);

/* Host form of the rule (no context, no GPU): frame i is frames[i][0 .. len[i]); order, trains
   and count as rxg_flow_trains_host wrote them.  Returns 0; -EINVAL: count or arena_used NULL,
   recs, frames or len NULL with n != 0, order NULL with cap_seg != 0, trains NULL with
   cap_trains != 0, arena NULL with arena_cap != 0, a bad rec_kind, unknown flag bits. */
int rxg_train_payload_host(const void *recs, uint32_t rec_kind, void *const *frames, const uint16_t *len,
                           uint32_t n, const uint32_t *order, uint64_t cap_seg, const rxg_flow_train *trains,
                           uint64_t cap_trains, const uint64_t count[4], uint32_t flags, void *arena,
                           uint64_t arena_cap, struct rxg_payload_msg *msgs, struct rxg_payload_msg *tmsgs,
                           uint64_t *arena_used);

/* ------------------------------------------------------------------------- */
/* A burst's ACKs planned per flow: one rxg_tx_seg per flow that received      */
/* data, and where the connection negotiated timestamps that ACK's option      */
/* block, both in the form rxg_tx_build_opt_dev takes.  The reference answers  */
/* once per poll, not per segment: tcp_established sets need_ack_now for a     */
/* segment with data or FIN (tcp_states.c:119-120) and the socket loop then    */
/* sends ptcb->tcp_flags = TCP_FLAG_ACK; sendtcpdata(ptcb, NULL, 0)            */
/* (socket_interface.c:214-218): a 20-byte TCP header, sent_seq = next_seq,    */
/* recv_ack = ptcb->ack, rx_win 12000 unswapped (tcp_out.c:157-207).  One ACK  */
/* per flow and burst that carries the flow's final ptcb->ack is that          */
/* coalescing.  Whether an ACK is sent stays the stack's decision, taken       */
/* against its own state at send time (rxg_ack_take below).                    */
/*                                                                             */
/* Inputs.  order, cap_seg, trains, cap_trains and train_count are the outputs */
/* of rxg_flow_trains_dev / _host for the burst of n frames; S' and T' are     */
/* rxg_train_payload_dev's: S' = min(train_count[0], cap_seg, n), T' =         */
/* min(train_count[1], cap_trains, n), T' = 0 when S' == 0.  rxopts (may be    */
/* NULL) are rxg_rx_opts_dev's n records for the same burst.  state[ntcb] is   */
/* the caller's table of rxg_ack_state, one entry per TCB.                     */
/*                                                                             */
/* Which flows get an ACK.  A flow is a maximal run of trains k < T' with one  */
/* tcb_idx (trains stand in tcb_idx order); its first train h is the one with  */
/* the lowest k, found by comparing train k with train k - 1:                  */
/* RXG_FTR_FLOW_FIRST is not trusted, so no list of trains gives one flow two  */
/* ACKs.  A flow whose tcb_idx is outside [0, ntcb) is counted in count[2] and */
/* its state is never read.  A flow whose state lacks RXG_AS_LIVE is counted   */
/* in count[1].  Every other flow gets an ACK; ACK a belongs to the a-th such  */
/* flow in train order.                                                        */
/*                                                                             */
/* The ACK's values.  If h carries RXG_FTR_HEAD: ack = trains[h].next_ack,     */
/* flagged RXG_ACK_ADVANCES, and RXG_ACK_FIN too when h carries RXG_FTR_FIN.   */
/* Otherwise ack = state.rcv_ack, flagged RXG_ACK_DUP: the burst brought the   */
/* flow nothing the window takes in order, the answer is a duplicate ACK.      */
/* seq = state.snd_nxt, win_raw = state.win_raw, tcp_flags = RXG_TCP_FLAG_ACK, */
/* data_len = 0, src_off = 0, pad = 0, flow = tcb_idx (the build's rxg_tx_flow */
/* table is indexed by TCB), ip_id = (uint16_t)(ip_id0 + a).                   */
/*                                                                             */
/* Options.  opts (may be NULL) is a table of opt_cap blocks the call writes   */
/* into; its first opt_base entries are the caller's own constant blocks and   */
/* are never touched.  opt_plain is 0..opt_base: 0 for sendtcpdata's 20-byte   */
/* header, or the 1-based index of a preloaded rxg_tx_opt_ref_ack block for    */
/* sendack's (tcp_out.c:350).  For a flow without RXG_AS_TS, or with opts      */
/* NULL, reserved = opt_plain.  For a flow with RXG_AS_TS: if opt_base + a <   */
/* opt_cap, opts[opt_base + a] is written as rxg_tx_opt_timestamp(tsval_now,   */
/* tsecr) writes it (len 12, the twelve bytes, every other byte of the 48      */
/* zero) and reserved = opt_base + a + 1; otherwise no block is written,       */
/* reserved = opt_plain, the ACK (valid without the echo) is flagged           */
/* RXG_ACK_NO_OPT and counted in count[3].  tsecr is the tsval of the HEAD     */
/* train's FIRST segment when the flow ADVANCES, rxopts is given, that segment */
/* -- packet order[trains[h].first], with trains[h].first < S' and the packet  */
/* < n -- has a record with RXG_O_TS: RFC 7323 section 4.3, an ACK for several */
/* segments echoes the earliest, the one that covers Last.ACK.sent.  In every  */
/* other case tsecr = state.ts_recent, and neither order nor rxopts is indexed */
/* out of range.  PAWS and the update of ts_recent stay the stack's.           */
/*                                                                             */
/* Outputs.  segs[a] (all 32 bytes defined) and acks[a] for a < cap; an ACK at */
/* or past cap writes neither them nor its option block, but is counted.       */
/* count is 4 words, WRITTEN: ACKs needed whatever cap is, flows not LIVE,     */
/* flows out of range, ACKs without their option block (whatever cap is).      */
/* n == 0 or T' == 0: count = {0, 0, 0, 0} and nothing else.  The output is a  */
/* pure function of the arguments: never of the grid, the stream, a mirror or  */
/* an earlier call.                                                            */
/*                                                                             */
/* Deliberately not in this call: SACK blocks (they need the window's pending  */
/* pairs, more per-connection state than a table of words); bare FINs without  */
/* data (no segment of any train: the stack acknowledges them itself);         */
/* delayed-ACK timing; frames (rxg_tx_build_opt_dev makes them from segs,      */
/* opts and a rxg_tx_flow table indexed by TCB, n = min(count[0], cap)).       */
/* ------------------------------------------------------------------------- */
typedef struct rxg_ack_state {   /* 16 bytes, tables 16-byte aligned */
    uint32_t snd_nxt;     /* ptcb->next_seq, host order                                       */
    uint32_t rcv_ack;     /* ptcb->ack as it stands before the burst                          */
    uint32_t ts_recent;   /* echoed when the burst gives no newer value                       */
    uint16_t win_raw;     /* stored unswapped, as tcp_out.c:190 (12000 = the reference's)     */
    uint16_t flags;       /* RXG_AS_*                                                         */
} rxg_ack_state;
#define RXG_AS_LIVE 0x1u  /* this TCB gets ACKs          */
#define RXG_AS_TS   0x2u  /* timestamps were negotiated  */

typedef struct rxg_ack {         /* 16 bytes, arrays 16-byte aligned */
    int32_t  tcb_idx;
    uint32_t ack, seq;    /* what segs[a] carries                                             */
    uint32_t flags_train; /* RXG_ACK_* in the low byte, the low 24 bits of h above them       */
} rxg_ack;
#define RXG_ACK_ADVANCES 0x01u /* ack is the HEAD train's next_ack                    */
#define RXG_ACK_DUP      0x02u /* ack is state.rcv_ack: a duplicate ACK               */
#define RXG_ACK_FIN      0x04u /* the acknowledged train ends in a FIN                */
#define RXG_ACK_NO_OPT   0x08u /* a timestamp flow whose block did not fit opt_cap    */

/* Asynchronous on `stream`, three launches: a lane per train decides whether the train is its
   flow's first and what becomes of the flow, with per-tile (256 trains) sums of ACKs, flows
   not LIVE and flows out of range; one workgroup scans the tile sums (rounds of 256 tiles
   with a carry) and writes count[0..2] and count[3] = 0; a lane per train again ranks its
   flow inside the tile on the tile's base and writes segs[a], acks[a] and the option block
   with 16-byte stores, adding its tile's ACKs without a block to count[3] (the one atomic:
   it decides no position).  No workgroup waits on another; train_count is read on the
   device only; rxg_config.max_blocks caps the grids and the output does not depend on them.
   The context owns the scratch (16 bytes per tile), grown on demand; one call at a time
   uses it, as for rxg_flow_trains_dev.
   -EINVAL: a NULL ctx, p, train_count, state or count; order NULL with cap_seg != 0, trains
   NULL with cap_trains != 0, segs or acks NULL with cap != 0; state, rxopts, opts, segs or
   acks not 16-, trains, train_count or count not 8-, order not 4-byte aligned; opt_plain >
   opt_base; opt_base > opt_cap; ntcb 0 or over RXG_FS_MAX_NTCB; flags != 0 (none is
   defined).  -ENOMEM: the scratch cannot be allocated; nothing is launched then.  A group's
   members are plain contexts for this call. */
typedef struct rxg_dev_ack_plan {
    const uint32_t *order;        /* dev: rxg_flow_trains_dev's order, cap_seg entries           */
    uint64_t cap_seg;
    const rxg_flow_train *trains; /* dev: its trains, cap_trains entries                         */
    uint64_t cap_trains;
    const uint64_t *train_count;  /* dev: its 4 count words, read on the device                  */
    uint32_t n;                   /* the burst's frames                                          */
    uint32_t ntcb;                /* 1 .. RXG_FS_MAX_NTCB: entries of state                      */
    const rxg_rx_opt *rxopts;     /* dev: rxg_rx_opts_dev's n records; may be NULL               */
    const rxg_ack_state *state;   /* dev, 16-byte aligned, ntcb entries                          */
    uint32_t flags;               /* 0                                                           */
    uint32_t tsval_now;           /* the TSval every written block carries                       */
    uint16_t ip_id0;
    uint16_t pad0;
    uint32_t opt_plain;           /* 0 .. opt_base                                               */
    uint32_t opt_base, opt_cap;   /* opt_base <= opt_cap                                         */
    rxg_tx_opt *opts;             /* dev, 16-byte aligned, opt_cap blocks; may be NULL           */
    rxg_tx_seg *segs;             /* dev, 16-byte aligned, cap entries                           */
    rxg_ack *acks;                /* dev, 16-byte aligned, cap entries                           */
    uint64_t cap;
    uint64_t *count;              /* dev, 4 words, WRITTEN                                       */
} rxg_dev_ack_plan;
int rxg_ack_plan_dev(rxg_ctx *ctx, const rxg_dev_ack_plan *p, void *stream);

/* Host form of the rule (no context, no GPU), for host-buffer bursts: the same struct with
   every pointer naming host memory (natural alignment suffices).  Returns 0; -EINVAL: the
   device call's list without the alignments. */
int rxg_ack_plan_host(const rxg_dev_ack_plan *p);

/* Using the prebuilt ACKs.  rxg_acks_attach names host copies of a call's `acks` (nacks =
   min(count[0], cap) entries, tcb_idx strictly ascending: attach verifies that) and of the
   frames built from its segs (ACK a at frames_host + a * stride) for the burst the next
   rxg_rx_replay call on this context replays.  Unlike the other attachments this one
   OUTLIVES that replay: the reference sends its ACK after the segments were handled
   (socket_interface.c:214).  It ends at the rxg_rx_replay after that one, at the next
   rxg_acks_attach, or at rxg_fini -- and with its own replay if that replay returns an
   error, from its argument checks or later: ACKs of a burst that was not replayed whole are
   never handed out.
   rxg_ack_take is called from the stack's ACK send, during that replay or after it
   returned, with the TCB and the stack's own next_seq and ack.  It returns 1 and sets
   *frame_out to the prebuilt frame exactly when (1) an attached ACK exists for tcb_idx;
   (2) its seq and ack equal snd_nxt and rcv_ack: a prebuilt ACK that no longer says what
   the stack's state says is never sent -- segments PushData refused, a handler that sent
   data meanwhile, a HEAD promise the caller voided; (3) the replay neither re-classified a
   packet to or from that TCB nor absorbed a mirror write to that slot (rxg_tcb_upsert /
   _remove / _set_state / _load, by a handler or between the burst and its replay), and no
   such write was made since the replay returned.  Writes after the replay are known until
   the next burst is launched on this context (its launch starts a new write log): call
   rxg_ack_take before that launch, or the seq / ack comparison alone stands between a slot
   that was given to another connection meanwhile and the old connection's frame.  It
   returns 0 otherwise, and before the replay has begun: the stack then builds its own ACK.
   -EINVAL: ctx or frame_out NULL (attach: ctx NULL, a NULL array or stride 0 with nacks
   != 0, tcb_idx not strictly ascending). */
int rxg_acks_attach(rxg_ctx *ctx, const rxg_ack *acks_host, void *frames_host, uint32_t stride, uint64_t nacks);
int rxg_ack_take(rxg_ctx *ctx, int32_t tcb_idx, uint32_t snd_nxt, uint32_t rcv_ack, void **frame_out);

/* ------------------------------------------------------------------------- */
/* Counters                                                                   */
/* ------------------------------------------------------------------------- */
int rxg_counters_reset(rxg_ctx *ctx, void *stream);
/* Synchronous read of the RXG_NCOUNTERS uint64 counters (the replica rows summed), after
   every burst of this context has finished, on whatever stream it was launched. */
int rxg_counters_read(rxg_ctx *ctx, uint64_t *out);
/* The device keeps RXG_COUNTER_ROWS rows of the counter block: 64 replicas the kernels add
   into (so that workgroups do not all add to one cache line) and one row of corrections
   written by rxg_rx_replay when it re-classifies packets; counter k = sum over rows. */
#define RXG_COUNTER_ROWS 65
/* Device address of the uint64[RXG_COUNTER_ROWS][RXG_NCOUNTERS] block: an in-place RCCL
   all-reduce (sum) over it followed by rxg_counters_read merges counters across GPUs.  The
   replay's corrections reach the block in the context's stream order: with the next mirror
   patch launch, or at the latest at rxg_counters_read, rxg_sync or this call (read the
   block after the context's stream, as for the kernels' own counts). */
void *rxg_counters_dev(rxg_ctx *ctx);

/* ------------------------------------------------------------------------- */
/* In-order hand-off (the side effects of etherin.c:21-35, ip.c:28-39,        */
/* tcp_in.c:47-72).  The caller supplies the reference's own functions.       */
/* ------------------------------------------------------------------------- */
typedef struct rxg_handoff_ops {
    void *user;
    void (*free_mbuf)(void *user, void *mbuf);                               /* main.c:206   */
    int (*arp_in)(void *user, void *mbuf);                                   /* arp.c:113    */
    /* ip.c:30-32: if (!get_mac(src)) add_mac(src, mac) */
    int (*get_mac)(void *user, uint32_t ipv4_host, unsigned char *mac_out);  /* arp.c:215    */
    int (*add_mac)(void *user, uint32_t ipv4_host, const unsigned char *mac);/* arp.c:282    */
    void (*send_reset)(void *user, void *ip_hdr, void *tcp_hdr);             /* tcp_out.c:103*/
    /* tcp_in.c:66-68 + 71: max_seq_received update and AdjustSendWindow(tcb, ack) */
    void (*on_segment)(void *user, int32_t tcb_idx, uint32_t seq, uint32_t ack);
    /* tcpswitch[state](tcb, tcp_hdr, ip_hdr, mbuf)             tcp_states.c:257-265 */
    int (*tcpswitch)(void *user, int32_t tcb_idx, uint8_t state, void *tcp_hdr, void *ip_hdr,
                     void *mbuf);
    /* The reference's rx counters, globals of tcp_in.c:18-19 exported at tcp_in.h:7,11.  The
       replay increments them where tcp_in does, in packet order: *tcpnopcb at every findtcb
       miss (tcp_in.c:47-48); *tcpchecksumerror only with RXG_OPS_VERIFY_TCP_CKSUM, at every
       TCP segment whose checksum fails (tcp_in.c:37-40).  NULL: not kept. */
    int *tcpnopcb;
    int *tcpchecksumerror;
    uint32_t flags;      /* RXG_OPS_* */
} rxg_handoff_ops;

/* rxg_handoff_ops.flags.  RXG_OPS_VERIFY_TCP_CKSUM turns on the block tcp_in.c:37-41 compiles
   out (`if(0)`): a TCP segment whose pseudo || segment checksum is not 0x0000 (record flag
   RXG_F_TCP_OK clear) is freed and counted in *tcpchecksumerror after ip_in's ARP learn,
   before findtcb -- no reset, no hand-off.  Off (0) is the reference as shipped. */
#define RXG_OPS_VERIFY_TCP_CKSUM 0x1u

/* Performs, in packet order, the side effects ether_in() would have performed for
   pkts[0..n) given their records.  frames[i] = the frame bytes of mbufs[i].  It must
   follow the burst (rxg_rx_burst or rxg_rx_burst_dev) of the same batch on this context;
   for rxg_rx_burst_dev the batch's device buffers must stay valid until it returns.

   Sequential equivalence: handlers (tcpswitch[], send_reset, ...) mirror their writes to
   tcbs[] with rxg_tcb_* as they happen.  When a handler changes the mirror, every later
   TCP packet of the batch whose classification can depend on the change (same dport as a
   changed slot; any packet that reached findtcb pass 2 after a slot was removed or NULL
   slots appeared) is re-classified on the GPU against the updated table before it is
   replayed, and the counters are corrected.  The composition rxg_rx_burst + rxg_rx_replay
   therefore equals `for (i<n) ether_in(mbufs[i])`.  After rxg_rx_bursts_dev the launch's
   bursts are replayed in order, one call each, and their composition equals ether_in over
   their concatenation.  recs: the burst's records as the launch wrote them, rec_stride =
   their kind (RXG_REC8: rxg_rec8[], RXG_REC16: rxg_rec16[], RXG_REC48: rxg_rec48[]).
   -EINVAL when n differs from the burst to be replayed or the launch failed after it started
   (nothing is replayed then). */
int rxg_rx_replay(rxg_ctx *ctx, const rxg_handoff_ops *ops, void *const *mbufs,
                  void *const *frames, const void *recs, uint32_t n, uint32_t rec_stride);

/* Cumulative replay statistics of the context: out[0] packets marked stale by in-burst
   table writes, out[1] of them re-classified from the host index, out[2] re-classified on
   the GPU, out[3] GPU re-classify launches. */
int rxg_replay_stats(rxg_ctx *ctx, uint64_t out[4]);

/* Per-packet form with ether_in's contract (etherin.c:12-37: takes ownership of the mbuf,
   returns 0): a burst of one through the GPU followed by its replay.  For a stack that
   keeps calling ether_in(m) one mbuf at a time -- its shim is
     int ether_in(struct rte_mbuf *m) {
         return rxg_ether_in(g_rxg, &g_ops, m, rte_pktmbuf_mtod(m, void *),
                             rte_pktmbuf_data_len(m)); }
   Each call is a GPU round trip; batching (rxg_rx_burst) is the fast path.  Negative on
   a HIP error (the mbuf is then not consumed). */
int rxg_ether_in(rxg_ctx *ctx, const rxg_handoff_ops *ops, void *mbuf, void *frame, uint16_t data_len);

/* ------------------------------------------------------------------------- */
/* Payload hand-off.  The reference copies each       */
/* in-order segment's payload into a mempool message for the socket ring:     */
/* tcp_established -> PushData (tcp_windows.c:341-358) -> AdjustPair (:42-110) */
/* -> PushDataInQueue (:112-136) -> GetData (:138-186).  rxg gathers the      */
/* payloads of a whole burst on the device; during rxg_rx_replay the stack's  */
/* PushData asks rxg_payload_take whether the window would deliver exactly    */
/* that payload as one message, and uses the gathered bytes if so.            */
/* ------------------------------------------------------------------------- */
enum rxg_payload_flag {
    RXG_PM_GATHERED = 0x01,     /* arena holds this frame's payload                          */
    RXG_PM_REF_OVERSIZE = 0x02, /* len >= 1000: the reference's GetData asserts here
                                   (tcp_windows.c:170, its Buffer[1000]); rxg delivers it   */
    RXG_PM_HOLE = 0x04          /* a train's message (rxg_train_payload_dev tmsgs): a segment
                                   of the train was not copied, its bytes are not in the span */
};

typedef struct rxg_payload_msg {
    uint64_t arena_off;  /* payload at arena + arena_off: 16-byte aligned (gather), or the
                            payload's offset in the frame pool (rxg_rx_burst_payload_dev), or
                            its place inside its train's span (rxg_train_payload_dev: any
                            alignment; a train's own message is 16-byte aligned)            */
    uint32_t len;        /* Length = datalen (tcp_states.c:111), bytes at frame + 34 +
                            (data_off >> 4) * 4 (tcp_windows.c:164-166); 0 if not gathered   */
    uint32_t flags;      /* RXG_PM_*                                                        */
} rxg_payload_msg;

typedef struct rxg_payload_out {
    void *arena;             /* dev; each message padded with zeros to 16 bytes             */
    uint64_t arena_cap;      /* bytes                                                       */
    rxg_payload_msg *msgs;   /* dev, one per frame of the burst (flags 0: not gathered)      */
    uint64_t *arena_used;    /* dev, 1 entry: bytes the burst's candidates need; frames past
                                arena_cap are not gathered.  UINT64_MAX (~0): the gather's
                                offset look-back timed out (a workgroup never published), so
                                arena offsets are unreliable; rxg_payload_take then refuses
                                every payload of the burst (the stack's own PushData runs)   */
} rxg_payload_out;

/* Gathers, for the LAST burst on this context (rxg_rx_burst or rxg_rx_burst_dev; its
   device batch and records must still be valid), the payload of every TCP segment
   (verdict DISPATCH, RST_NOPCB or RST_LISTEN_NONSYN -- the replay may turn the latter into
   a DISPATCH) with datalen > 0 and the payload inside the frame.  Packet order;
   asynchronous on `stream`.  o->msgs and o->arena_used must stay valid until the burst's
   replay is done: the first rxg_payload_take after the gather copies them to the host.
   One gather is in flight per context: a gather waits (on the device) for the previous
   one, whatever streams they were issued on. */
int rxg_payload_gather_dev(rxg_ctx *ctx, const rxg_payload_out *o, void *stream);

/* The burst and its payload hand-off in ONE pass over the frames (rxg_rx_burst_dev followed
   by rxg_payload_gather_dev reads every payload byte twice).  The same records and counters
   as rxg_rx_burst_dev, and one message per frame for exactly the frames the gather takes
   (same len and flags; the message bytes are the same payload bytes), but each payload stays
   where its frame puts it: the arena has the frame pool's geometry.  For a candidate frame i
   the 64-byte lines of [frames + 64*off64[i] + start, + datalen) are written, unchanged, at
   the same offsets from `arena` (start = 34 + data_off*4), and msgs[i].arena_off = 64*off64[i]
   + start (not 16-byte aligned); other frames' lines are not written.  `arena` must hold
   64*(max off64[i]) + len rounded up to 64 bytes, and be 64-byte aligned; msgs 16-byte
   aligned (128-byte alignment measured 8 % faster than 64).  arena NULL: the hand-off by
   reference -- nothing is copied, each message names its payload in the frame pool itself
   (arena_off from `frames`), for a stack that keeps the pool's buffers until the socket side
   has consumed the messages (the reference's planned zero-copy path, currentstatus:9).
   rxg_payload_take then answers from these messages, as after a gather.  Asynchronous on
   `stream`. */
typedef struct rxg_payload_slots {
    void *arena;            /* dev: the pool's geometry (see above), or NULL         */
    rxg_payload_msg *msgs;  /* dev, b->n messages                                   */
} rxg_payload_slots;
int rxg_rx_burst_payload_dev(rxg_ctx *ctx, const rxg_dev_batch *b, const rxg_payload_slots *p, void *stream);
/* The same for one fixed-stride burst (rxg_rx_bursts_strided_dev's frame placement: frame i at
   64-byte slot b->slot0 + i * stride64 of the pool, msgs[i].arena_off = 64 * that slot + start). */
int rxg_rx_burst_strided_payload_dev(rxg_ctx *ctx, const void *frames, uint32_t stride64,
                                     const rxg_dev_strided_burst *b, uint32_t rec_kind,
                                     const rxg_payload_slots *p, void *stream);

/* Receive-window mirror: ReceiveWindow.CurrentSequenceNumber of tcbs[idx] and whether its
   SeqPairs list is non-empty (tcp_windows.h:37-44).  The stack calls it wherever it
   writes them itself: tcp_listen (tcp_states.c:182) and after its own PushData when
   rxg_payload_take refused.  rxg_tcb_remove / rxg_tcb_load forget the slot's window. */
int rxg_rcv_set(rxg_ctx *ctx, int32_t idx, uint32_t cur_seq, uint32_t pairs_pending);

/* Called from the stack's PushData(mbuf, tcp, Length, ptcb) (tcp_windows.c:341) while
   rxg_rx_replay runs the handlers of a packet of the gathered burst.  Returns 1 when the
   reference would deliver exactly this packet's payload as one message -- the mirror says
   the window of tcbs[idx] holds no pairs and CurrentSequenceNumber == seq, the payload was
   gathered with this length, and PushData's duplicate test (cur > seq + Length, u32) does
   not drop it.  Then *msg describes the message, the mirror advances to seq + Length, and
   the stack does what AdjustPair + GetData + PushDataInQueue would have: ptcb->ack =
   seq + Length + (FIN ? 1 : 0), CurrentSequenceNumber = seq + Length, enqueue a message of
   Length bytes (the gathered ones), free the mbuf.  Returns 0 otherwise (the stack runs its
   own PushData, then rxg_rcv_set); negative on error. */
int rxg_payload_take(rxg_ctx *ctx, int32_t idx, uint32_t seq, uint32_t length, rxg_payload_msg *msg);

/* ------------------------------------------------------------------------- */
/* Synthetic traffic (bench / tests): Eth + IPv4 (IHL 5) + TCP (doff 5, ACK)   */
/* frames with valid checksums, SURVEY.md §8(d).                               */
/* ------------------------------------------------------------------------- */
typedef struct rxg_synth_params {
    uint64_t seed;        /* payload / header PRNG seed                          */
    uint32_t n;           /* frames                                              */
    uint32_t nflows;      /* flow f: src 10.(f>>16).(f>>8).(f), sport 1024+f%64511 */
    uint32_t dst_ip_host; /* 192.168.78.2 = 0xC0A84E02 (config.h:8)             */
    uint16_t dport;       /* 80                                                  */
    uint16_t mix;         /* 0: all frames len_a; 1: IMIX 64/576/1500 at 7:4:1    */
    uint16_t len_a;       /* frame length when mix == 0                          */
    uint16_t pad;
} rxg_synth_params;

/* Fills off64/len (dev) and frames (dev) for p->n frames, packed at 64-byte aligned
   starts; returns the arena bytes used in *arena_bytes.  Frame flows are uniform over
   nflows (stored per frame in flow_out, dev, may be NULL). */
int rxg_synth_dev(rxg_ctx *ctx, const rxg_synth_params *p, void *frames, uint64_t frames_cap,
                  uint32_t *off64, uint16_t *len, uint32_t *flow_out, uint64_t *arena_bytes,
                  void *stream);
/* Host helper: the arena bytes rxg_synth_dev needs for p. */
uint64_t rxg_synth_arena_bytes(const rxg_synth_params *p);

/* ------------------------------------------------------------------------- */
/* Device memory helpers (so ctypes/C callers need no other HIP binding).      */
/* ------------------------------------------------------------------------- */
int rxg_dev_alloc(rxg_ctx *ctx, uint64_t bytes, void **out);
int rxg_dev_free(rxg_ctx *ctx, void *p);
int rxg_host_alloc_pinned(rxg_ctx *ctx, uint64_t bytes, void **out);
int rxg_host_free_pinned(rxg_ctx *ctx, void *p);
/* Zero-copy batches.  Host memory from rxg_host_alloc_pinned, or caller memory registered
   here (e.g. the mbuf pool's hugepages: hipHostRegister, mapped), may be passed to
   rxg_rx_burst_dev / rxg_tx_cksum_dev as `frames`, `off64`, `len` and `out` through its
   device alias: the kernel reads (and for tx rewrites in place) the frames over PCIe, with
   no staging copy.  rxg_tx_cksum_dev on host frames writes back only the rewritten first
   line of each frame, not the frame (C5).  The alias is valid until
   rxg_host_unregister. */
int rxg_host_register(rxg_ctx *ctx, void *host, uint64_t bytes, void **dev_alias);
int rxg_host_unregister(rxg_ctx *ctx, void *host);
int rxg_memcpy_h2d(rxg_ctx *ctx, void *dst, const void *src, uint64_t bytes, void *stream);
int rxg_memcpy_d2h(rxg_ctx *ctx, void *dst, const void *src, uint64_t bytes, void *stream);
int rxg_memset_dev(rxg_ctx *ctx, void *dst, int value, uint64_t bytes, void *stream);
int rxg_stream_sync(rxg_ctx *ctx, void *stream);

/* Event timing on a stream (bench): returns ms between two recorded events. */
typedef struct rxg_event rxg_event;
int rxg_event_create(rxg_ctx *ctx, rxg_event **out);
int rxg_event_record(rxg_ctx *ctx, rxg_event *e, void *stream);
int rxg_event_elapsed_ms(rxg_ctx *ctx, rxg_event *a, rxg_event *b, float *ms);
int rxg_event_destroy(rxg_ctx *ctx, rxg_event *e);

/* Last error text of this thread (static storage). */
const char *rxg_last_error(void);

/* ------------------------------------------------------------------------- */
/* Groups: several GPUs behind one rx loop.  The reference   */
/* runs one rx lcore calling ether_in per packet (main.c:391-399); a group     */
/* keeps that single loop and spreads each burst over its members.            */
/*  - every member holds a full replica of the TCB / ARP / receive-window      */
/*    mirrors: the rxg_group_* mirror calls apply to all of them;             */
/*  - rxg_group_rx_burst cuts the burst into one contiguous shard per member   */
/*    (ceil(n/ndev) frames, so cfg->max_batch is per shard), runs the shards   */
/*    concurrently (one worker thread per member, kept for the group's life)   */
/*    and returns the records in packet order;                                 */
/*  - rxg_group_rx_burst_dev takes a burst already in GPU-visible memory as    */
/*    one shard per member and launches every member at once (no host copy);   */
/*  - rxg_group_rx_replay replays the shards in packet order.  Handlers mirror */
/*    their tcbs[] writes with rxg_group_tcb_* (not the member calls), so a    */
/*    later member's replay sees them and re-classifies what they affect: the  */
/*    composition equals ether_in over the whole burst, as for one context.    */
/* Members are plain contexts (rxg_group_member) for everything else: device    */
/* batches, payload gathers, timing.  Group calls are made from the rx thread;  */
/* rxg_group_tcb_post is the any-thread exception (member rxg_tcb_post is not  */
/* used on a group: per-member queues could order two posts differently).      */
/* ------------------------------------------------------------------------- */
typedef struct rxg_group rxg_group;
/* One context per devices[i] (the same device may repeat), each with *cfg's sizes. */
int rxg_group_init(const int32_t *devices, uint32_t ndev, const rxg_config *cfg, rxg_group **out);
int rxg_group_fini(rxg_group *g);
uint32_t rxg_group_size(rxg_group *g);
rxg_ctx *rxg_group_member(rxg_group *g, uint32_t i);
int rxg_group_tcb_upsert(rxg_group *g, int32_t idx, const rxg_tcb_tuple *t);
int rxg_group_tcb_remove(rxg_group *g, int32_t idx);
int rxg_group_tcb_set_state(rxg_group *g, int32_t idx, uint8_t state);
int rxg_group_tcb_load(rxg_group *g, const rxg_tcb_tuple *tcbs, const uint8_t *live, int32_t ntcb);
/* Any thread: one lock-free queue for the whole group (the members apply posts in one
   order), drained at the start of rxg_group_rx_burst or by rxg_group_tcb_drain. */
int rxg_group_tcb_post(rxg_group *g, const rxg_tcb_op *op);
int rxg_group_tcb_drain(rxg_group *g);
int rxg_group_arp_load(rxg_group *g, const uint32_t *ipv4_host, uint32_t n);
int rxg_group_arp_learned(rxg_group *g, uint32_t ipv4_host);
int rxg_group_arp_disable(rxg_group *g);
int rxg_group_rcv_set(rxg_group *g, int32_t idx, uint32_t cur_seq, uint32_t pairs_pending);
int rxg_group_rx_burst(rxg_group *g, const rxg_pkt_view *pkts, uint32_t n, uint32_t rec_kind,
                       void *out_host);
/* Device-resident group burst (contiguous batches to the GPUs, the host
   replays in global packet order), replacing main.c:391-399's loop for frames the caller
   already has in GPU-visible memory.  shards[i] (nshards = group size) is member i's
   contiguous share of the burst, in packet order (shard 0 first; any n, 0 included), with
   the rxg_dev_batch rules of rxg_rx_burst_dev in memory member i's GPU reads: its HBM, or
   host memory registered on member i (rxg_host_register; e.g. the mbuf pool registered on
   every member).  Every shard has the same rec_kind.  Each member classifies its shard
   against its replica of the mirror as it stands at the call; the launches are asynchronous,
   one per member on its own stream, so the shards run concurrently.  rxg_group_sync waits
   for them; rxg_group_rx_replay then replays n = sum of the shards' n records, laid out in
   packet order with that stride, exactly as after rxg_group_rx_burst (each member's shard
   buffers must stay valid until the replay returns). */
int rxg_group_rx_burst_dev(rxg_group *g, const rxg_dev_batch *shards, uint32_t nshards);
/* Waits for every member's stream (rxg_sync on each). */
int rxg_group_sync(rxg_group *g);
int rxg_group_rx_replay(rxg_group *g, const rxg_handoff_ops *ops, void *const *mbufs,
                        void *const *frames, const void *recs, uint32_t n, uint32_t rec_stride);
/* rxg_payload_take on the member whose shard is being replayed (0 outside a replay);
   each member's rxg_payload_gather_dev covers its own shard. */
int rxg_group_payload_take(rxg_group *g, int32_t idx, uint32_t seq, uint32_t length, rxg_payload_msg *msg);
/* Index of the member being replayed, -1 outside rxg_group_rx_replay. */
int32_t rxg_group_replaying(rxg_group *g);
int rxg_group_counters_reset(rxg_group *g);
/* The members' counters summed: an RCCL all-reduce (sum, uint64) of the members' counter
   blocks over xGMI when the members are distinct GPUs (one communicator per member,
   ncclCommInitAll at the first call), else summed on the host (members sharing a GPU). */
int rxg_group_counters_read(rxg_group *g, uint64_t *out);
/* 1 when rxg_group_counters_read merges with RCCL, 0 when on the host; negative on error.
   RCCL is loaded at the first merge over distinct GPUs (dlopen of librccl.so): librxg.so
   does not depend on it, and a host without it merges on the host (same sums). */
int rxg_group_counters_rccl(rxg_group *g);
/* Why the merge is on the host (empty when RCCL is used or not decided yet). */
const char *rxg_group_counters_rccl_why(rxg_group *g);
/* Last error of a group call on this thread (member errors carry their text). */
const char *rxg_group_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* RXG_H */
