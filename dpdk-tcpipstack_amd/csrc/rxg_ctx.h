// rxg_ctx.h — the context behind the rxg C ABI (include/rxg.h), shared by the host-side
// translation units (internal: not installed, not part of the ABI):
//   rxg_host.cpp    context, TCB / ARP mirrors, launched bursts, counters, and
//                   HipTablePort, the device side of rxg_tablesync.h
//   rxg_ops.cpp     the operations on a burst beside its classification: tx checksums, segment
//                   build, reset build, transmit planner, received options, flow summary,
//                   flow trains, train payload, ACK plan
//   rxg_tablesync.h the device tables and the order of their writes against the kernels that
//                   read them (patch ring, carried list, mirror_ev, reader events): HIP-free
//   rxg_server.cpp  latency mode (the persistent server kernel) and host-buffer bursts
//   rxg_replay.cpp  the per-packet replay into the caller's handlers, the payload hand-off,
//                   the C entry points of what a replay hands out, ether_in
//   rxg_attached.h  what a replay hands out and the rules it is answered by (ReplayAttached),
//                   the receive-window mirror (RcvWindow): HIP-free
//   rxg_replaylog.h which packets a table write made stale and how each is fixed (WriteSet,
//                   ReplayLog): HIP-free
//   rxg_util.cpp    synthetic frames, memory and event helpers
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "rxg.h"
#include "rxg_attached.h"
#include "rxg_common.h"
#include "rxg_kernels.h"
#include "rxg_mirror.h"
#include "rxg_opqueue.h"
#include "rxg_packpool.h"
#include "rxg_replaylog.h"
#include "rxg_srvfsm.h"
#include "rxg_tablesync.h"

// Everything below is internal to librxg.so: hidden, never exported.
#pragma GCC visibility push(hidden)

// Sets the calling thread's rxg_last_error text and returns code (rxg_host.cpp).
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_OK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(-EIO, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,      \
                        __LINE__);                                                          \
    } while (0)

using rxg::DevBuf;

// The latency-mode server's device side as rxg::SrvFsm sees it (rxg_srvfsm.h); defined in
// rxg_server.cpp.
struct SrvPort {
    rxg_ctx *c;
    unsigned long long done() const;
    bool exited() const;
    void write(unsigned long long q);
    void cancel(unsigned long long q);
    void request_stop();
    int launch();
    void sync();
};

// The device side of the table synchronisation as rxg::TableSync sees it (rxg_tablesync.h:
// the Port's contract); defined in rxg_host.cpp, the only HIP calls on those paths.
struct HipTablePort {
    using Stream = hipStream_t;
    using Event = hipEvent_t;
    rxg_ctx *c = nullptr;
    Stream stream() const;
    int event_create(Event *e, bool reader);
    void event_destroy(Event e);
    int record(Event e, Stream s);
    int stream_wait(Stream s, Event e);
    int host_wait(Event e);
    int sync();
    int patch_alloc(rxg::MirrorPatch **p, uint32_t cap, bool dev);
    int patch_free(rxg::MirrorPatch *p, bool dev);
    void patch_write(rxg::MirrorPatch *dst, const rxg::MirrorPatch *src, uint32_t n, bool dev);
    int patch_launch(const rxg::MirrorPatch *list, uint32_t n, const DevBuf &buckets, const DevBuf &listen,
                     const DevBuf &arp);
    int table_resize(DevBuf &b, size_t bytes);
    int table_upload(DevBuf &b, const void *src, size_t bytes);
};

// Scratch memory of the context that one call at a time uses (an operation's launches share it
// and the next call overwrites it).  The rule, for calls on any streams: a call waits, on its
// stream, for the previous call's last launch (the event, recorded at the end of every call,
// even after a failed launch: whatever part of it was enqueued is waited for); before a buffer
// is replaced by a larger one the host waits for that launch instead.
struct SerialScratch {
    const char *who;      // the entry point, for its error texts
    DevBuf buf[3] = {};
    hipEvent_t ev = nullptr;
    bool open = false;    // begin() without its end()

    // b (one of buf) grown to `bytes`, never shrunk.  zero: the new memory is zeroed on st.
    // -ENOMEM when it cannot be had (b is then empty).
    int grow(DevBuf &b, size_t bytes, bool zero, hipStream_t st)
    {
        if (b.p && b.bytes >= bytes) return 0;
        if (ev) HIP_OK(hipEventSynchronize(ev));
        if (b.p) HIP_OK(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
        const size_t want = std::max<size_t>(bytes, 256);
        if (hipMalloc(&b.p, want) != hipSuccess) {
            (void)hipGetLastError();
            b.p = nullptr;
            return fail(-ENOMEM, "%s: %zu bytes of device memory", who, want);
        }
        b.bytes = want;
        if (zero) HIP_OK(hipMemsetAsync(b.p, 0, want, st));
        return 0;
    }
    // before the call's first launch on st
    int begin(hipStream_t st)
    {
        if (ev) HIP_OK(hipStreamWaitEvent(st, ev, 0));
        else HIP_OK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        open = true;
        return 0;
    }
    // after its last; returns the launches' error as the entry point's code (a call that
    // never began, one of no frames, records nothing)
    int end(hipStream_t st, hipError_t launch_error)
    {
        if (open) {
            open = false;
            HIP_OK(hipEventRecord(ev, st));
        }
        HIP_OK(launch_error);
        return 0;
    }
    void destroy()
    {
        for (DevBuf &b : buf)
            if (b.p) (void)hipFree(b.p);
        if (ev) (void)hipEventDestroy(ev);
    }
};

// The operations whose launch grid the context works out once, at init (rxg_ctx::op_grid).
enum GridOp { kGridPay, kGridTxBuild, kGridTxBuildOpt, kGridTxReset, kGridRxOpts, kGridTxPlan, kGridFlowSum, kGridFlowTrain,
              kGridTrainPay, kGridAckPlan, kGridOps };

struct rxg_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t max_blocks = 0;        // rxg_config.max_blocks: grid cap (0 = occupancy grid)
    // grids by operation, set at init (rxg_init says what each is); 0: unknown (grid_cap)
    uint32_t op_grid[kGridOps] = {512};
    // occupancy grids by [the by-reference hand-off's kernel][grid_slot(record kind)] (grid_for)
    uint32_t grid[2][4] = {};
    rxg::PackPool pack_pool;  // rxg_rx_burst's packing threads

    // tcbs[] writes posted by other threads (rxg_tcb_post), applied by the rx thread
    rxg::MpscRing<rxg_tcb_op> posted{RXG_TCB_QUEUE_CAP};

    // host mirror of tcbs[0..ntcb) and the device words each write changes (rxg_mirror.h)
    rxg::TcbMirror mir;

    // the device tables and the order of their writes against their readers (rxg_tablesync.h)
    rxg::TableSync<HipTablePort> tables;
    // HDP_MEM_COHERENCY_FLUSH_CNTL (hipDeviceProp_t::hdpMemFlushCntl; null if the runtime
    // gives none): host writes through the BAR are flushed to memory before a kernel reads them
    volatile uint32_t *hdp_flush = nullptr;

    unsigned long long *counters = nullptr;
    // the replays' counter corrections not yet on the device: added by the next mirror patch
    // launch, or by counters_add at the next read / sync / rxg_counters_dev (flush_delta)
    int64_t pend_delta[RXG_NCOUNTERS] = {};
    bool pend = false;

    // mirror changes since the last clear, for rxg_rx_replay's re-classification
    uint64_t gen = 0;
    rxg::WriteSet touched;
    bool replay_on_device = false;  // RXG_CFG_REPLAY_ON_DEVICE
    rxg::ReplayLog replay;          // the running (or last) replay's staleness rule and records

    // the last burst's device batch (re-classification reads it again)
    // The last launch's bursts (one, or several of one frame pool: rxg_rx_bursts_dev) and
    // the one a replay / gather refers to next (last_off .. last_recs below).
    struct BurstRef {
        const uint32_t *off64;  // nullptr for a fixed-stride burst (slot0, stride64)
        const uint16_t *len;
        uint32_t n;
        const uint8_t *recs;
        uint32_t slot0 = 0, stride64 = 0;
    };
    std::vector<BurstRef> last_bursts;
    uint32_t replay_cursor = 0;
    // writes absorbed by the replays of this launch's earlier bursts (they came after every
    // burst of the launch was classified)
    rxg::WriteSet launch_writes;
    const uint8_t *last_frames = nullptr;
    const uint32_t *last_off = nullptr;  // nullptr: a fixed-stride burst (burst_offsets)
    uint32_t last_slot0 = 0, last_stride64 = 0;
    DevBuf d_soff;                       // a fixed-stride burst's offsets, written on demand
    uint32_t soff_slot0 = 0, soff_stride64 = 0, soff_n = 0;  // what d_soff holds (n 0: nothing),
    hipStream_t soff_stream = nullptr;                        // written on this stream
    const uint16_t *last_len = nullptr;
    uint32_t last_n = 0;
    bool burst_ok = false;  // the last burst was launched (device) / completed (host buffers)
    const uint8_t *last_recs = nullptr;  // the burst's records (device) and their size
    uint32_t last_stride = 0;
    DevBuf d_sel, d_fix;

    // payload hand-off: the receive-window mirror (rxg_rcv_set), the gathers' look-back words
    rxg::RcvWindow rcv;
    DevBuf d_pg_status, d_pg_ticket;
    unsigned long long pg_tickets = 0;  // workgroups the gathers have launched so far
    uint32_t pg_epoch = 0;
    // The messages rxg_payload_take answers from: those of the last gather, train payload or fused
    // burst (pm_handoff records where they are), fetched into a pinned host copy at the first take.
    struct PayloadMsgs {
        const rxg_payload_msg *dev = nullptr;  // the call's descriptors (device)
        const uint64_t *used = nullptr;        // its arena_used (device); NULL: no look-back to time out
        uint32_t n = 0;                        // 0: the selected burst has none
        hipEvent_t ev = nullptr;               // recorded after the call's last launch
        bool pending = false;                  // host not fetched yet for this call
        bool poisoned = false;                 // its look-back timed out: no payload is handed out
        rxg_payload_msg *host = nullptr;       // pinned, host_cap entries
        uint32_t host_cap = 0;
    } pm;
    rxg::ReplayAttached attached;  // what the replay hands out, and the packet it is at

    // rxg_tx_reset_dev: the slice counts its three launches share (buf[0])
    SerialScratch rst{"rxg_tx_reset_dev"};
    // rxg_tx_plan_dev: the tile sums its launches share (buf[0])
    SerialScratch txp{"rxg_tx_plan_dev"};
    // rxg_flow_sums_dev: the dense accumulator and the touched bitmap (all zero between calls)
    // and the tile counts (buf[kFsAcc .. kFsTiles])
    enum { kFsAcc, kFsBits, kFsTiles };
    SerialScratch fs{"rxg_flow_sums_dev"};
    bool fs_dirty = false;  // a launch failed part-way: both are zeroed again before the next

    // rxg_flow_trains_dev: the pairs' two buffers, the segments' meta and the trains' starts, and
    // the counts its launches hand on (buf[kFtPairs .. kFtCounts]); no content is kept
    enum { kFtPairs, kFtMeta, kFtCounts };
    SerialScratch ft{"rxg_flow_trains_dev"};

    // rxg_train_payload_dev: the trains' offsets and the tile sums (buf[0]); no content is kept
    SerialScratch tp{"rxg_train_payload_dev"};
    // rxg_ack_plan_dev: the tile sums (buf[0]); no content is kept
    SerialScratch ak{"rxg_ack_plan_dev"};

    // ARP mirror (host set + device open-addressing table, rxg_mirror.h)
    bool arp_enabled = false;
    rxg::ArpMirror arp;
    std::unordered_map<uint32_t, int> arp_since_burst;  // learned after the last burst

    // host-buffer burst staging
    uint32_t max_batch = 0;
    uint64_t max_bytes = 0;
    uint8_t *h_arena = nullptr;
    uint32_t *h_off = nullptr;
    uint16_t *h_len = nullptr;
    uint8_t *d_arena = nullptr;
    uint32_t *d_off = nullptr;
    uint16_t *d_len = nullptr;
    uint8_t *d_out = nullptr;
    uint8_t *h_out = nullptr;        // pinned records of zero-copy host bursts
    uint64_t zc_bytes = 64ull << 20; // host bursts up to this many staged bytes: zero-copy

    // latency-mode server (rxg_server_*): a persistent kernel on its own
    // stream; the host-burst staging in device memory the host writes through the BAR
    // (dev = true) or in coherent host memory; the mailbox likewise (mdev), answers and
    // records in host memory
    struct Server {
        bool on = false;        // configured (the kernel may have exited idle: relaunched on demand)
        rxg::SrvFsm<SrvPort> fsm;  // Down / Up / Failed (rxg_srvfsm.h)
        rxg::SrvReq req{};      // the request SrvPort::write posts
        // its inline descriptors (kSrvInlineDesc): mailbox words 16-39, SrvMbox::ioff / ilen
        alignas(16) unsigned long long idesc[rxg::kSrvPollWords - 16] = {};
        bool dev = false;       // arena / off / len in device memory (host writes only)
        bool mdev = false;      // mbox in device memory (large BAR, no RXG_SRV_HOST_MAILBOX)
        hipStream_t st = nullptr;
        rxg::SrvMbox *mbox = nullptr;  // host-written words: seq, request, stop
        rxg::SrvMbox *ret = nullptr;   // server-written words: done, exited (host memory; = mbox if !mdev)
        rxg::SrvCtl *ctl = nullptr;
        uint8_t *arena = nullptr;
        uint32_t *off = nullptr;
        uint16_t *len = nullptr;
        uint8_t *out = nullptr;
        std::vector<uint32_t> h_off;  // host copies of the packed offsets (device staging is
        std::vector<uint16_t> h_len;  // write-only from the host: a read would cross PCIe)
        uint32_t rec_kind = 0, blocks = 1, max_frames = 0;
        uint64_t max_bytes = 0, idle_ticks = 0;
        unsigned long long seq = 0;
        uint64_t synced_writes = 0;    // table writes the host has waited for (host_wait_writes)
    } srv;
};

// Host stores into device memory through the BAR (write-combined), made visible to the next
// kernel: the CPU's write-combining buffers drained (sfence), the GPU's HDP write path flushed
// (its flush register), then a read of the last word written -- a PCIe read completes only
// after every posted write before it, the flush among them (the ROCm runtime's own recipe
// for kernel arguments in device memory).  `last` NULL: no readback.
void bar_publish(const rxg_ctx *c, const volatile uint32_t *last);

inline constexpr size_t kCounterBytes = (size_t)RXG_COUNTER_ROWS * RXG_NCOUNTERS * sizeof(uint64_t);

struct rxg_event {
    hipEvent_t e;
};

inline int set_device(rxg_ctx *c) { HIP_OK(hipSetDevice(c->device)); return 0; }

inline int ensure(DevBuf &b, size_t bytes)
{
    if (b.bytes >= bytes && b.p) return 0;
    if (b.p) HIP_OK(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    size_t want = std::max<size_t>(bytes, 256);
    HIP_OK(hipMalloc(&b.p, want));
    b.bytes = want;
    return 0;
}

inline hipStream_t pick(rxg_ctx *c, void *s) { return s ? (hipStream_t)s : c->stream; }

// The device tables as the kernels read them (DevTable, rxg_kernels.h).
inline rxg::DevTable table_view(const rxg_ctx *c)
{
    rxg::DevTable t = c->tables.view();
    if (!c->arp_enabled) t.arp_mask = 0u;
    t.arp_flags = c->arp_enabled ? (rxg::kArpOn | (c->arp.has_zero ? rxg::kArpZero : 0u)) : 0u;
    return t;
}

inline hipStream_t HipTablePort::stream() const { return c->stream; }

// A launch's grid: the max_blocks override, else the occupancy grid of the kernel for
// rec_kind (0: tx) and whether it is the by-reference hand-off's.
inline int grid_slot(uint32_t rec_kind)
{
    return rec_kind == RXG_REC8 ? 1 : rec_kind == RXG_REC16 ? 2 : rec_kind == RXG_REC48 ? 3 : 0;
}
// (occupancy: a grid worked out at init, 0 where the device's properties could not be read)
inline uint32_t grid_cap(const rxg_ctx *c, uint32_t occupancy)
{
    return c->max_blocks ? c->max_blocks : occupancy ? occupancy : 1024u;
}
inline uint32_t grid_for(const rxg_ctx *c, uint32_t rec_kind, bool by_ref = false)
{
    return grid_cap(c, c->grid[by_ref][grid_slot(rec_kind)]);
}

// rxg_host.cpp: the mirror upload, the replay bookkeeping of a burst set and its offsets.
// tcb_push: the device TCB tables brought up to date with the mirror (nothing if they are).
int tcb_push(rxg_ctx *c);
void select_burst(rxg_ctx *c, uint32_t j);
int begin_bursts(rxg_ctx *c, const void *frames, const rxg_dev_burst *bursts, uint32_t k, uint32_t rec_kind,
                 const char *who, uint32_t stride64 = 0, bool carry = false);
int burst_offsets(rxg_ctx *c, hipStream_t st, const uint32_t **out);
// The n messages at msgs (device), written by what was just launched on st, are what
// rxg_payload_take answers from next; used: that call's arena_used (device), or NULL.
int pm_handoff(rxg_ctx *c, hipStream_t st, const rxg_payload_msg *msgs, const uint64_t *used, uint32_t n);
// the pending counter corrections (rxg_ctx::pend_delta) to the device, on c->stream
int flush_delta(rxg_ctx *c);

// the counter block's row of replay corrections (rxg.h RXG_COUNTER_ROWS: the last)
inline unsigned long long *correction_row(rxg_ctx *c)
{
    return c->counters + (size_t)(RXG_COUNTER_ROWS - 1) * RXG_NCOUNTERS;
}

inline bool rec_kind_ok(uint32_t k) { return k == RXG_REC8 || k == RXG_REC16 || k == RXG_REC48; }

// The alignment of a burst's records: the kernels read and write them with 8- or 16-byte
// vector accesses.
inline uintptr_t rec_align(uint32_t rec_kind) { return rec_kind == RXG_REC8 ? 8u : 16u; }

// The strided mode of a frame source (off64 NULL: frame i at slot slot0 + i * stride64) must
// name a stride and stay inside 2^32 slots.  burst >= 0: the text names that burst of a set.
inline int check_frame_src(const char *who, const uint32_t *off64, uint32_t slot0, uint32_t stride64, uint32_t n,
                           int burst = -1)
{
    if (off64) return 0;
    if (!stride64) return fail(-EINVAL, "%s: stride64 0", who);
    if (n && (uint64_t)slot0 + (uint64_t)(n - 1u) * stride64 > 0xFFFFFFFFull) {
        char which[24] = "";
        if (burst >= 0) snprintf(which, sizeof which, " burst %d:", burst);
        return fail(-EINVAL, "%s:%s slot0 + (n - 1) * stride64 exceeds 2^32 - 1 slots", who, which);
    }
    return 0;
}

#pragma GCC visibility pop
