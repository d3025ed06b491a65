// rxg_kernels.h — host-side launch interface of rxg_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "rxg_common.h"

namespace rxg {

struct MirrorPatch;  // rxg_mirror.h

// One launch classifies up to kMaxBursts bursts whose frames share one pool (`frames`):
// burst k's frame i is at frames + 64 * off64[i], its record at out + i * record size.
constexpr uint32_t kMaxBursts = 32;
struct LaunchBurst {
    const uint32_t *off64;  // strided launches (LaunchRx::stride64 != 0): unused
    const uint16_t *len;
    uint32_t n;            // >= 1 (empty bursts are not launched)
    uint8_t *out;          // records (receive), unused for tx
    uint32_t slot0;        // strided launches: the 64-byte slot of the burst's frame 0
};

struct LaunchRx {
    const uint8_t *frames;
    const uint32_t *sel;   // optional selection list into burst 0 (re-classification), else nullptr
    const LaunchBurst *bursts;
    uint32_t nbursts;      // 1 .. kMaxBursts
    int mode;              // 16 / 48: receive records of that size; 0: tx checksum generate
    DevTable table;
    unsigned long long *counters;
    uint32_t max_blocks;   // grid cap (grid-stride over 64-frame slices)
    uint32_t stride64;     // nonzero: frame i of a burst at slot slot0 + i * stride64 (no off64[])
    uint8_t *pay_arena;    // non-null (with pay_msgs): the payload hand-off fused in (one burst,
    rxg_payload_msg *pay_msgs;  //   record kind 8 / 16 / 48; rxg_rx_burst_payload_dev)
    // mirror patches the launch applies before its first probe, in place of a patch launch
    // before it (rxg_host.cpp launch_bursts; the list in device memory, kLaunchPatchMax at most)
    const MirrorPatch *ipatch;
    uint32_t nipatch;
};

struct LaunchSynth {
    uint8_t *frames;
    uint32_t *off64;
    uint16_t *len;
    uint32_t *flow;
    uint64_t seed;
    uint64_t arena_bytes;
    uint32_t n, nflows, dst_ip, dport, mix, len_a;
};

struct LaunchPayload {
    const uint8_t *frames;
    const uint32_t *off64;
    const uint16_t *len;
    const uint8_t *recs;   // the burst's records (rxg_rec16 / rxg_rec48, `stride` bytes apart)
    uint32_t stride;
    uint32_t n;
    rxg_payload_msg *msgs;
    uint8_t *arena;
    uint64_t arena_cap;
    unsigned long long *status;       // payload_blocks(n) look-back words (any content)
    unsigned long long *ticket;       // workgroup ticket counter, kept across launches
    unsigned long long ticket_base;   // its value before this launch
    unsigned long long *used;         // 1 entry
    uint32_t epoch;                   // 1 .. 2^30-1, new for every launch on `status`
};

hipError_t launch_rx(const LaunchRx &L, hipStream_t st);

// Where an operation on a burst finds its frames: frame i is at frames + 64 * off64[i], or with
// off64 null (strided mode) at slot slot0 + i * stride64; len[i] is its length.  A member of
// the launch structs below and of their kernels' arguments (rxg_dev.h frame_slot).
struct FrameSrc {
    const uint8_t *frames;
    const uint32_t *off64;
    const uint16_t *len;
    uint32_t slot0, stride64;
};

// Latency mode (rxg_server_*): a persistent set of workgroups that classifies one burst after
// another.  The host posts a request in a mailbox of fine-grained (coherent) host memory and
// spins on its `done`; workgroup 0 polls the mailbox and hands each request to the others
// through `SrvCtl` in device memory.  No launch and no stream synchronisation per burst.
struct SrvReq {
    const uint8_t *frames;   // device-visible: HBM or mapped host memory
    const uint32_t *off64;
    const uint16_t *len;
    uint8_t *out;            // records of the server's kind
    uint32_t n;
    uint32_t flags;          // kSrvInlineDesc: the descriptors are in the mailbox (SrvMbox::ioff / ilen);
                             // kSrvLarge: a frame over 64 bytes (host bursts)
    DevTable table;          // the mirror as of the post
};
// Host bursts of up to kSrvInline frames carry their descriptors in the mailbox, on the lines
// the server's poll reads with the request: its frame loads then wait for no descriptor load
// (one dependent device-memory trip less per served burst).
constexpr uint32_t kSrvInline = 32;
constexpr uint32_t kSrvInlineDesc = 1u;
// A host burst holding a frame over 64 bytes: a request of 3..gridDim slices then runs one
// slice per workgroup, each shared by the workgroup's four waves (rx_body, HISTORY.md §9.R4).
constexpr uint32_t kSrvLarge = 2u;
// Device memory written through the BAR (large-BAR GPUs, whole lines per post) or coherent
// host memory; `done` / `exited` are read from the server's return block (host memory, may
// be a second SrvMbox).  The first 320 bytes (words 0-39) are what the host writes and the
// server polls, read whole by one wave instruction (40 lanes x 8 bytes): a request is taken
// when seq is new and `check` is srv_check of seq, the request words and, for a request with
// kSrvInlineDesc, the inline descriptor words 16-39.  Write-combined stores reach the device
// as whole lines or in parts, in any order between lines until the host's fence: the check
// word is what makes a snapshot holding words of two requests fail (it is then polled again),
// not the order of the stores.  The server's words are on a line of their own.
struct alignas(128) SrvMbox {
    unsigned long long seq;       // host: number of the request posted
    SrvReq req;
    unsigned long long check;     // host: srv_check(seq, req, ioff, ilen)
    unsigned long long stop;      // host: nonzero = exit
    unsigned long long hpad[2];
    uint32_t ioff[kSrvInline];    // words 16-31: off64 of an inline request's frames
    uint16_t ilen[kSrvInline];    // words 32-39: their lengths
    alignas(128) unsigned long long done;  // server: number of the last request finished
    unsigned long long exited;    // server: nonzero once the kernel has left its loop
};
constexpr int kSrvPollWords = 40;  // words 0-39: the request and its inline descriptors
static_assert(sizeof(SrvReq) == 88, "mailbox layout");
static_assert(offsetof(SrvMbox, check) == 96 && offsetof(SrvMbox, stop) == 104 && offsetof(SrvMbox, ioff) == 128 &&
                  offsetof(SrvMbox, ilen) == 256 && offsetof(SrvMbox, done) == 384,
              "mailbox layout");
// Word i of the mailbox (0 = seq, 1-11 = the request, 16-39 = inline descriptors) mixed with
// its position; the check word is the XOR of the mixed words (a splitmix64 finaliser: any mix
// of old and new words changes it but with probability 2^-64).
__host__ __device__ inline unsigned long long srv_mix(unsigned i, unsigned long long w)
{
    unsigned long long z = w + (unsigned long long)(i + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// desc: words 16-39 of an inline request (nullptr otherwise)
inline unsigned long long srv_check(unsigned long long seq, const SrvReq &r, const unsigned long long *desc)
{
    unsigned long long w[sizeof(SrvReq) / 8];
    __builtin_memcpy(w, &r, sizeof w);
    unsigned long long h = srv_mix(0u, seq);
    for (unsigned i = 0; i < sizeof(SrvReq) / 8; ++i) h ^= srv_mix(i + 1u, w[i]);
    if (desc)
        for (unsigned i = 16; i < (unsigned)kSrvPollWords; ++i) h ^= srv_mix(i, desc[i - 16]);
    return h;
}
struct SrvCtl {                   // device memory
    unsigned long long go;        // number << 16 | participants of the request the workgroups run
                                  // (kSrvStop: exit); the host sets done << 16 before a launch
    unsigned int fin;             // participants finished with the current request (the last
                                  // one resets it to 0 before publishing `done`)
    unsigned int pad;
    SrvReq req;                   // the current request, read by its participants only
};
constexpr unsigned long long kSrvStop = ~0ull;
struct LaunchServer {
    SrvMbox *mbox;                  // host-written words (host or device memory)
    SrvMbox *ret;                   // done / exited (host memory); nullptr = mbox
    SrvCtl *ctl;
    unsigned long long *counters;
    unsigned long long idle_ticks;  // wall-clock ticks without a request before the kernel exits
    uint32_t blocks;
    int mode;                       // record kind 8 / 16 / 48
};
hipError_t launch_server(const LaunchServer &L, hipStream_t st);
// rxg_payload.hip: gather of the burst's candidate payloads (one launch + a memset)
hipError_t launch_payload(const LaunchPayload &P, hipStream_t st, uint32_t *tickets_used);
uint32_t payload_blocks(uint32_t n);
// rxg_txbuild.hip: transmit segment build (rxg_tx_build_dev, rxg_tx_build_opt_dev), one launch
struct LaunchTxBuild {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const rxg_tx_flow *flows;
    uint32_t nflows;
    uint32_t n;
    const rxg_tx_seg *segs;
    uint8_t *frames;
    const uint32_t *off64;  // nullptr: frame i at slot slot0 + i * stride64
    uint32_t slot0, stride64;
    uint16_t *len;
    unsigned long long *stats;  // {built, skipped}, added to; may be nullptr
    uint32_t max_blocks;        // grid cap (grid-stride over 64-segment slices); 0 = none
    bool with_opts;             // rxg_tx_build_opt_dev: rxg_tx_seg.reserved names a block of opts
    const rxg_tx_opt *opts;     // nopts blocks (16-byte aligned), or nullptr with nopts 0
    uint32_t nopts;
};
hipError_t launch_tx_build(const LaunchTxBuild &B, hipStream_t st);
int tx_build_blocks_per_cu(bool with_opts);  // resident 256-thread workgroups per CU of its kernel
// rxg_txreset.hip: reset replies from a burst's records (rxg_tx_reset_dev): a count pass, a
// one-workgroup scan and a build pass on `st` (n == 0: *count = 0 only)
struct LaunchTxReset {
    FrameSrc src;
    uint32_t n;
    uint32_t rec_kind;
    const uint8_t *recs;
    uint8_t *out;
    uint32_t *idx;
    unsigned long long cap;
    unsigned long long *count;
    uint32_t *counts;       // tx_reset_count_bytes(n) bytes, shared by the three launches
    uint32_t ip_id0;
    uint8_t src_mac[6];
    uint32_t max_blocks;    // grid cap of the count and build passes (grid-stride); 0 = none
};
hipError_t launch_tx_reset(const LaunchTxReset &R, hipStream_t st);
size_t tx_reset_count_bytes(uint32_t n);  // the slice-count buffer a call of n frames needs
int tx_reset_blocks_per_cu();  // resident 256-thread workgroups per CU of the build pass
// rxg_txplan.hip: sends cut into segment descriptors (rxg_tx_plan_dev): a count pass, a
// one-workgroup scan, an offsets pass and an expand pass on `st` (nsends == 0: count = {0, 0}
// and first[0] = 0 only)
struct LaunchTxPlan {
    const rxg_tx_send *sends;
    uint32_t nsends, mss;
    const uint32_t *send_opt;   // nullptr: no send names a block
    const rxg_tx_opt *opts;     // nopts blocks, or nullptr with nopts 0
    uint32_t nopts;
    rxg_tx_seg *segs;
    unsigned long long cap;
    unsigned long long *first;  // nsends + 1 entries
    uint32_t *next_seq;         // may be nullptr
    unsigned long long *count;  // {total, refused sends}
    void *tiles;                // tx_plan_tile_bytes(nsends) bytes, shared by the launches
    uint32_t max_blocks;        // grid cap of the count, offsets and expand passes; 0 = 2^16
};
hipError_t launch_tx_plan(const LaunchTxPlan &P, hipStream_t st);
size_t tx_plan_tile_bytes(uint32_t nsends);  // the tile buffer a call of nsends sends needs
int tx_plan_blocks_per_cu();  // resident 256-thread workgroups per CU of the expand pass
// rxg_rxopt.hip: the TCP options of a burst's segments (rxg_rx_opts_dev), one launch on `st`
// (n == 0: none)
struct LaunchRxOpts {
    FrameSrc src;
    uint32_t n;
    uint32_t rec_kind;
    const uint8_t *recs;
    uint8_t *out;           // n rxg_rx_opt records
    uint32_t max_blocks;    // grid cap (grid-stride over 64-frame slices); 0 = none
};
hipError_t launch_rx_opts(const LaunchRxOpts &R, hipStream_t st);
int rx_opts_blocks_per_cu();  // resident 256-thread workgroups per CU of its kernel
// rxg_flowsum.hip: a burst summarised per flow (rxg_flow_sums_dev): the accumulation, the
// touched bitmap's per-tile counts, their one-workgroup scan and the expansion on `st`
// (n == 0: count = {0, 0, 0} only)
struct FlowSumAcc {         // one accumulator entry; all zero between calls
    uint32_t frames, max_seq, max_ack;
    uint32_t first_enc;     // max of ~i over the counted frames (0: none)
    uint32_t last_enc;      // max of i + 1
    uint32_t data_frames, flags_or, pad;
    unsigned long long data_bytes;
};
static_assert(sizeof(FlowSumAcc) == 40, "accumulator entry");
constexpr uint32_t kFsTileWords = 64;                  // bitmap words per count tile (one per lane)
constexpr uint32_t kFsTileTcbs = kFsTileWords * 32u;   // TCBs per count tile
constexpr uint32_t kFsScanLanes = 1024;                // tiles per round of the scan
struct LaunchFlowSum {
    FrameSrc src;           // frames may be nullptr for RXG_REC48
    uint32_t n;
    uint32_t rec_kind;
    const uint8_t *recs;
    uint32_t ntcb, flags;
    rxg_flow_sum *out;
    unsigned long long cap;
    unsigned long long *count;  // 3 words
    FlowSumAcc *acc;            // flow_sum_bytes(ntcb) bytes, all zero
    uint32_t *bits;             // flow_sum_bits_bytes(ntcb) bytes, all zero: two 64-bit words of
                                // left-out frames (count[1], count[2]), then the touched bitmap
    uint32_t *tiles;            // flow_sum_tile_bytes(ntcb) bytes, any content
    uint32_t max_blocks;        // grid cap of the count and expand passes; 0 = none
    uint32_t acc_blocks;        // grid of the accumulation (its waves carry a flow across slices)
};
hipError_t launch_flow_sum(const LaunchFlowSum &F, hipStream_t st);
size_t flow_sum_bytes(uint32_t ntcb);
size_t flow_sum_bits_bytes(uint32_t ntcb);
size_t flow_sum_tile_bytes(uint32_t ntcb);
// rxg_flowtrain.hip: a burst's data segments grouped by flow and cut into trains
// (rxg_flow_trains_dev): the select, the radix sort's passes and the cut on `st` (n == 0:
// count = {0, 0, 0, 0} only)
constexpr uint32_t kFtTile = 1024;         // pairs per tile of the sort and of the cut (a workgroup's)
constexpr uint32_t kFtScanLanes = 1024;    // lanes of the one-workgroup scans
constexpr uint32_t kFtScanPer = 16;        // entries per lane and round of a scan
struct LaunchFlowTrain {
    FrameSrc src;           // frames may be nullptr for RXG_REC48
    uint32_t n;
    uint32_t rec_kind;
    const uint8_t *recs;
    uint32_t ntcb, flags;
    const uint32_t *cur_seq;    // may be nullptr
    uint32_t *order;
    unsigned long long cap_seg;
    rxg_flow_train *trains;
    unsigned long long cap_trains;
    unsigned long long *count;  // 4 words
    void *pairs;                // flow_train_pair_bytes(n) bytes, any content
    void *meta;                 // flow_train_meta_bytes(n) bytes, any content
    uint32_t *counts;           // flow_train_count_bytes(n) bytes, any content
    uint32_t max_blocks;        // grid cap of every pass but the scans; 0 = 2^16
};
hipError_t launch_flow_train(const LaunchFlowTrain &F, hipStream_t st);
uint32_t flow_train_passes(uint32_t ntcb);  // 8-bit passes of the sort: as many as ntcb - 1 has bytes
size_t flow_train_pair_bytes(uint32_t n);
size_t flow_train_meta_bytes(uint32_t n);
size_t flow_train_count_bytes(uint32_t n);
int flow_train_blocks_per_cu();  // resident 256-thread workgroups per CU of the scatter pass
// rxg_trainpay.hip: a burst's payload gathered by train (rxg_train_payload_dev): msgs zeroed, the
// taking trains' padded sizes per tile, their one-workgroup scan, the trains' offsets and the
// copy on `st` (n == 0: *used = 0 only)
constexpr uint32_t kTpTile = 256;        // trains per tile of the offsets, segments per tile of the copy
constexpr uint32_t kTpScanLanes = 256;   // tile sums per round of the one-workgroup scan
struct LaunchTrainPay {
    FrameSrc src;
    uint32_t n;
    uint32_t rec_kind;
    const uint8_t *recs;
    const uint32_t *order;
    unsigned long long cap_seg;
    const rxg_flow_train *trains;
    unsigned long long cap_trains;
    const unsigned long long *count;  // the flow-train call's 4 words, read on the device
    uint32_t flags;
    uint8_t *arena;
    unsigned long long arena_cap;
    rxg_payload_msg *msgs, *tmsgs;    // either may be nullptr
    unsigned long long *used;         // 1 entry
    void *scratch;                    // train_pay_scratch_bytes(n, cap_trains) bytes, any content
    uint32_t max_blocks;              // grid cap of every pass but the scan; 0 = 2^16
};
hipError_t launch_train_pay(const LaunchTrainPay &P, hipStream_t st);
size_t train_pay_scratch_bytes(uint32_t n, unsigned long long cap_trains);
int train_pay_blocks_per_cu();  // resident 256-thread workgroups per CU of the copy
// rxg_ackplan.hip: a burst's ACKs planned per flow (rxg_ack_plan_dev): the flows' classes summed per
// tile, their one-workgroup scan and the descriptors, records and option blocks on `st` (no
// train readable -- n, cap_seg or cap_trains 0: count = {0, 0, 0, 0} only)
constexpr uint32_t kAkTile = 256;        // trains per tile
constexpr uint32_t kAkScanLanes = 256;   // tile sums per round of the one-workgroup scan
struct LaunchAckPlan {
    const uint32_t *order;
    unsigned long long cap_seg;
    const rxg_flow_train *trains;
    unsigned long long cap_trains;
    const unsigned long long *train_count;  // the flow-train call's 4 words, read on the device
    uint32_t n, ntcb;
    const rxg_rx_opt *rxopts;         // may be nullptr
    const rxg_ack_state *state;
    uint32_t tsval_now, ip_id0, opt_plain, opt_base, opt_cap;
    rxg_tx_opt *opts;                 // may be nullptr
    rxg_tx_seg *segs;
    rxg_ack *acks;
    unsigned long long cap;
    unsigned long long *count;        // 4 words
    void *scratch;                    // ack_plan_scratch_bytes(n, cap_trains) bytes, any content
    uint32_t max_blocks;              // grid cap of the count and emit passes; 0 = 2^16
};
hipError_t launch_ack_plan(const LaunchAckPlan &P, hipStream_t st);
size_t ack_plan_scratch_bytes(uint32_t n, unsigned long long cap_trains);
int ack_plan_blocks_per_cu();  // resident 256-thread workgroups per CU of the emit pass
// resident 256-thread workgroups per CU of the production kernel of `mode` (by_ref: the
// by-reference payload hand-off's, whose record ring also stages the messages)
int rx_blocks_per_cu(int mode, bool by_ref = false);
hipError_t launch_synth(const LaunchSynth &L, hipStream_t st);
// off[i] = slot0 + i * stride64, i < n (a fixed-stride burst's offsets as a list)
hipError_t launch_strided_offsets(uint32_t *off, uint32_t n, uint32_t slot0, uint32_t stride64, hipStream_t st);
// rxg_mirror.h patches (n of them, host-visible memory) applied to the device mirror tables
// Replay counter corrections (two's complement: a negative delta wraps the uint64 sum)
struct CounterDelta {
    int64_t v[RXG_NCOUNTERS];
};
hipError_t launch_counters_add(unsigned long long *row, const CounterDelta &d, hipStream_t st);

// crow != nullptr: the launch also adds *delta to that counter row (the replay's pending
// corrections, rxg_replay.cpp), saving their own launch
hipError_t launch_mirror_patch(const MirrorPatch *p, uint32_t n, uint4 *buckets, int32_t *listen, uint32_t *arp,
                               hipStream_t st, unsigned long long *crow = nullptr, const CounterDelta *delta = nullptr);

}  // namespace rxg
