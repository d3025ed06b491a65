// rxg_host.cpp — host side of the rxg C ABI (include/rxg.h): the context, mirrors, launched
// bursts and counters (the other entry points: rxg_ops.cpp, rxg_server.cpp, rxg_replay.cpp,
// rxg_util.cpp; the context itself: rxg_ctx.h).
//
// Owns one GPU context: its stream, the device TCB mirror (rebuilt from the host mirror
// whenever a rxg_tcb_* call made it dirty), the counter block, and the pinned staging used
// by the host-buffer entry points.  There is no CPU compute path: without a usable HIP
// device every compute entry point returns -ENODEV / -EIO.
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <immintrin.h>
#include <vector>


#include "rxg_ctx.h"

using namespace rxg;

static_assert(sizeof(rxg_rec16) == 16, "rxg_rec16 layout");
static_assert(sizeof(rxg_rec48) == 48, "rxg_rec48 layout");
static_assert(sizeof(rxg_tcb_tuple) == 20, "rxg_tcb_tuple layout");

// ------------------------------------------------------------------------ errors ---
static thread_local char g_err[512];

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *rxg_last_error(void) { return g_err; }

void bar_publish(const rxg_ctx *c, const volatile uint32_t *last)
{
    _mm_sfence();
    if (c->hdp_flush) {
        *c->hdp_flush = 1u;
        _mm_sfence();
    }
    if (last) (void)*last;
}

extern "C" int rxg_abi_version(void) { return RXG_ABI_VERSION; }

extern "C" int rxg_init(const rxg_config *cfg, rxg_ctx **out)
{
    if (!out) return fail(-EINVAL, "rxg_init: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(-ENODEV, "rxg_init: no HIP device (%s)", hipGetErrorString(e));
    rxg_ctx *c = new rxg_ctx();
    c->device = cfg ? cfg->device : 0;
    if (c->device < 0 || c->device >= ndev) {
        delete c;
        return fail(-EINVAL, "rxg_init: device %d of %d", cfg ? cfg->device : 0, ndev);
    }
    int rc = set_device(c);
    if (rc) { delete c; return rc; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess) {
        // one generation of resident workgroups per CU (grid-stride over slices)
        const uint32_t cus = (uint32_t)prop.multiProcessorCount;
        for (int kind : {0, (int)RXG_REC8, (int)RXG_REC16, (int)RXG_REC48}) {  // 0: tx
            c->grid[0][grid_slot(kind)] = cus * (uint32_t)rx_blocks_per_cu(kind);
            if (kind) c->grid[1][grid_slot(kind)] = cus * (uint32_t)rx_blocks_per_cu(kind, true);
        }
        // the fused burst + payload hand-off moves as many bytes out as in: 2 workgroups per CU
        // (8 waves) measured faster than the occupancy grid's 3 (C3 621 against 627 us, C4 174
        // against 177)
        c->op_grid[kGridPay] = cus * 2u;
        // the occupancy grids of the operations' kernels (rxg_ops.cpp; the reset's is its build
        // pass's, the planner's its expand pass's)
        c->op_grid[kGridTxBuild] = cus * (uint32_t)tx_build_blocks_per_cu(false);
        c->op_grid[kGridTxBuildOpt] = cus * (uint32_t)tx_build_blocks_per_cu(true);
        c->op_grid[kGridTxReset] = cus * (uint32_t)tx_reset_blocks_per_cu();
        c->op_grid[kGridRxOpts] = cus * (uint32_t)rx_opts_blocks_per_cu();
        c->op_grid[kGridTxPlan] = cus * (uint32_t)tx_plan_blocks_per_cu();
        // rxg_flow_sums_dev's accumulation: one workgroup per CU.  Every workgroup ends with one
        // set of atomics on its carried flow, and atomics on one line run one after the other:
        // 256 workgroups measured faster than 1 024 on every shape
        c->op_grid[kGridFlowSum] = cus;
        // rxg_flow_trains_dev: the occupancy grid of its scatter pass
        c->op_grid[kGridFlowTrain] = cus * (uint32_t)flow_train_blocks_per_cu();
        // rxg_train_payload_dev: the occupancy grid of its copy
        c->op_grid[kGridTrainPay] = cus * (uint32_t)train_pay_blocks_per_cu();
        // rxg_ack_plan_dev: the occupancy grid of its emit pass
        c->op_grid[kGridAckPlan] = cus * (uint32_t)ack_plan_blocks_per_cu();
    }
    // a large BAR: the mirror's patch lists live in device memory the host writes directly,
    // and a burst launch carries its own (launch_bursts)
    int large_bar = 0;
    bool bar_lists = false;
    if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, c->device) == hipSuccess && large_bar) {
        void *probe = nullptr;  // and host-writable device memory can be had
        if (hipExtMallocWithFlags(&probe, 4096, hipDeviceMallocFinegrained) == hipSuccess) {
            (void)hipFree(probe);
            bar_lists = true;
        }
        hipDeviceProp_t hp;
        if (hipGetDeviceProperties(&hp, c->device) == hipSuccess) c->hdp_flush = hp.hdpMemFlushCntl;
    }
    if (cfg) {
        c->replay_on_device = (cfg->flags & RXG_CFG_REPLAY_ON_DEVICE) != 0;
        c->max_blocks = cfg->max_blocks;
        if (cfg->zc_bytes) c->zc_bytes = cfg->zc_bytes;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(-EIO, "rxg_init: hipStreamCreate failed");
    }
    c->tables.port.c = c;
    if (c->tables.init(bar_lists, cfg && (cfg->flags & RXG_CFG_STREAMS_OUTLIVE_WRITES) != 0)) {
        rxg_fini(c);
        return fail(-EIO, "rxg_init: hipEventCreate failed");
    }
    if (hipMalloc(&c->counters, kCounterBytes) != hipSuccess ||
        hipMemset(c->counters, 0, kCounterBytes) != hipSuccess) {
        rxg_fini(c);
        return fail(-ENOMEM, "rxg_init: counters");
    }
    // the ARP bucket every lane reads while the mirror is off (classify_finish issues the
    // ARP probe unconditionally)
    DevBuf &arp0 = c->tables.d_arp;
    if (ensure(arp0, 256) || hipMemset(arp0.p, 0, arp0.bytes) != hipSuccess) {
        rxg_fini(c);
        return fail(-ENOMEM, "rxg_init: ARP mirror");
    }
    c->max_batch = cfg ? cfg->max_batch : 0;
    c->max_bytes = cfg ? cfg->max_bytes : 0;
    if (c->max_batch) {
        uint64_t ab = c->max_bytes ? c->max_bytes : (uint64_t)c->max_batch * 2048u;
        c->max_bytes = ab;
        if (hipHostMalloc((void **)&c->h_arena, ab, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&c->h_off, c->max_batch * 4u, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc((void **)&c->h_len, c->max_batch * 2u, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&c->d_arena, ab) != hipSuccess ||
            hipMalloc(&c->d_off, c->max_batch * 4u) != hipSuccess ||
            hipMalloc(&c->d_len, c->max_batch * 2u) != hipSuccess ||
            hipMalloc(&c->d_out, (size_t)c->max_batch * 48u) != hipSuccess ||
            hipHostMalloc((void **)&c->h_out, (size_t)c->max_batch * 48u, hipHostMallocDefault) != hipSuccess) {
            rxg_fini(c);
            return fail(-ENOMEM, "rxg_init: staging for %u frames / %llu bytes", c->max_batch,
                        (unsigned long long)ab);
        }
    }
    *out = c;
    return 0;
}

extern "C" int rxg_fini(rxg_ctx *c)
{
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    // A server kernel that missed its time limit may still be resident, reading the tables and
    // counters and writing the staging and records.  Stop is retried for a bounded time (each
    // try waits exit_timeout); if the kernel still has not exited, everything it can reach is
    // deliberately leaked -- the context included -- rather than freed under it: -EIO.
    int src = rxg_server_stop(c);
    for (int t = 0; src && t < 4; ++t) src = rxg_server_stop(c);
    if (src)
        return fail(-EIO, "rxg_fini: the server kernel has not exited; the context and every buffer it can "
                          "reach are left allocated (leaked)");
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    (void)c->tables.wait_readers(true);  // table readers still running on caller streams
    for (DevBuf *b : {&c->tables.buckets, &c->tables.listen, &c->d_sel, &c->d_fix, &c->tables.d_arp, &c->d_pg_status,
                      &c->d_pg_ticket, &c->d_soff})
        if (b->p) (void)hipFree(b->p);
    for (SerialScratch *s : {&c->rst, &c->txp, &c->fs, &c->ft, &c->tp, &c->ak}) s->destroy();
    if (c->pm.host) (void)hipHostFree(c->pm.host);
    if (c->pm.ev) (void)hipEventDestroy(c->pm.ev);
    c->tables.destroy();
    if (c->counters) (void)hipFree(c->counters);
    if (c->h_arena) (void)hipHostFree(c->h_arena);
    if (c->h_off) (void)hipHostFree(c->h_off);
    if (c->h_len) (void)hipHostFree(c->h_len);
    if (c->d_arena) (void)hipFree(c->d_arena);
    if (c->d_off) (void)hipFree(c->d_off);
    if (c->d_len) (void)hipFree(c->d_len);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->h_out) (void)hipHostFree(c->h_out);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

extern "C" int rxg_sync(rxg_ctx *c)
{
    if (!c) return fail(-EINVAL, "rxg_sync: ctx NULL");
    if (int rc = flush_delta(c)) return rc;
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" void *rxg_stream(rxg_ctx *c) { return c ? (void *)c->stream : nullptr; }


// -------------------------------------------------------------------- TCB mirror ---
// What a write to tcbs[idx] can change for packets of the burst being replayed: pass 1 of
// packets with the slot's tuple, pass 2 of packets on its dport if it is (or was) LISTENING.
static void note_slot(rxg_ctx *c, int32_t idx)
{
    if (idx >= c->mir.ntcb() || !c->mir.live[idx]) return;
    const rxg_tcb_tuple &t = c->mir.tcb[idx];
    TupleKey k;
    if (tcb_key(t, k)) c->touched.keys.push_back(k);
    if (t.state == RXG_LISTENING && port_in_range(t.dport)) c->touched.listen.push_back(t.dport);
}

extern "C" int rxg_tcb_upsert(rxg_ctx *c, int32_t idx, const rxg_tcb_tuple *t)
{
    if (!c || !t) return fail(-EINVAL, "rxg_tcb_upsert: NULL argument");
    if (t->state >= RXG_TCP_STATES) return fail(-EINVAL, "rxg_tcb_upsert: state %u", t->state);
    if (idx < 0 || idx >= kMaxTcbs) return fail(-EINVAL, "tcb index %d outside 0..%d", idx, kMaxTcbs - 1);
    const int32_t min_null = c->mir.min_null;
    note_slot(c, idx);  // the old tuple / listener
    c->mir.upsert(idx, *t);
    note_slot(c, idx);  // the new ones
    // NULL slots appearing (old Ntcb .. idx-1) or disappearing (a removed slot reused) move
    // min_null, the pass-2 NULL-slot flag of later packets
    if (c->mir.need_rebuild || c->mir.min_null != min_null) c->touched.pass2 = true;
    c->tables.tcb_changed();
    c->gen++;
    return 0;
}

extern "C" int rxg_tcb_remove(rxg_ctx *c, int32_t idx)
{
    if (!c) return fail(-EINVAL, "rxg_tcb_remove: ctx NULL");
    if (idx < 0 || idx >= c->mir.ntcb())
        return fail(-EINVAL, "rxg_tcb_remove: index %d outside Ntcb %d", idx, c->mir.ntcb());
    const int32_t min_null = c->mir.min_null;
    note_slot(c, idx);
    c->mir.remove(idx);
    if (c->mir.need_rebuild || c->mir.min_null != min_null) c->touched.pass2 = true;
    c->rcv.forget(idx);  // FreeWindow
    c->tables.tcb_changed();
    c->gen++;
    return 0;
}

extern "C" int rxg_tcb_set_state(rxg_ctx *c, int32_t idx, uint8_t state)
{
    if (!c) return fail(-EINVAL, "rxg_tcb_set_state: ctx NULL");
    if (state >= RXG_TCP_STATES) return fail(-EINVAL, "rxg_tcb_set_state: state %u", state);
    if (idx < 0 || idx >= c->mir.ntcb() || !c->mir.live[idx])
        return fail(-EINVAL, "rxg_tcb_set_state: index %d is not a live slot", idx);
    note_slot(c, idx);
    c->mir.set_state(idx, state);
    note_slot(c, idx);
    c->tables.tcb_changed();
    c->gen++;
    return 0;
}

extern "C" int rxg_tcb_load(rxg_ctx *c, const rxg_tcb_tuple *tcbs, const uint8_t *live, int32_t ntcb)
{
    if (!c || ntcb < 0 || (ntcb > 0 && !tcbs)) return fail(-EINVAL, "rxg_tcb_load: bad arguments");
    if (ntcb > kMaxTcbs) return fail(-EINVAL, "rxg_tcb_load: %d TCBs exceed %d", ntcb, kMaxTcbs);
    for (int32_t i = 0; i < ntcb; ++i)
        if ((!live || live[i]) && tcbs[i].state >= RXG_TCP_STATES)
            return fail(-EINVAL, "rxg_tcb_load: slot %d state %u", i, tcbs[i].state);
    c->mir.load(tcbs, live, ntcb);
    c->tables.tcb_changed();
    c->touched.all = true;
    c->gen++;
    c->rcv.clear();
    return 0;
}

extern "C" int32_t rxg_tcb_count(rxg_ctx *c) { return c ? c->mir.ntcb() : -EINVAL; }

extern "C" int rxg_flow_partition(rxg_ctx *c, uint32_t part, uint32_t nparts)
{
    if (!c) return fail(-EINVAL, "rxg_flow_partition: ctx NULL");
    if (nparts == 0 || nparts > RXG_RSS_RETA_SIZE || part >= nparts)
        return fail(-EINVAL, "rxg_flow_partition: part %u of %u", part, nparts);
    if (c->mir.part == part && c->mir.nparts == nparts) return 0;
    c->mir.part = part;
    c->mir.nparts = nparts;
    c->mir.need_rebuild = true;  // the whole table, as after rxg_tcb_load
    c->tables.tcb_changed();
    c->touched.all = true;
    c->gen++;
    return 0;
}

extern "C" int rxg_flow_partition_get(rxg_ctx *c, uint32_t *part, uint32_t *nparts)
{
    if (!c || !part || !nparts) return fail(-EINVAL, "rxg_flow_partition_get: NULL argument");
    *part = c->mir.part;
    *nparts = c->mir.nparts;
    return 0;
}

extern "C" uint32_t rxg_rss_hash(const uint8_t tuple12[12]) { return tuple12 ? rss_toeplitz(tuple12, 12) : 0u; }

extern "C" int rxg_flow_part_of(const uint8_t *f, uint32_t len, uint32_t nparts)
{
    if ((!f && len) || nparts == 0 || nparts > RXG_RSS_RETA_SIZE)
        return fail(-EINVAL, "rxg_flow_part_of: frame NULL or nparts %u outside 1..%u", nparts, RXG_RSS_RETA_SIZE);
    uint8_t b[38] = {0};
    std::memcpy(b, f, std::min<uint32_t>(len, 38u));
    // ether_in's demux and ip_in's protocol test (etherin.c:12-37, ip.c:19-42): only TCP
    // over IPv4 reaches findtcb
    if (b[12] != 0x08 || b[13] != 0x00 || b[23] != RXG_IPPROTO_TCP) return 0;
    return (int)rss_queue(rss_toeplitz12(b + 26), nparts);
}

extern "C" int64_t rxg_tcb_keys(rxg_ctx *c) { return c ? (int64_t)c->mir.nkeys() : -EINVAL; }

extern "C" int rxg_tcb_post(rxg_ctx *c, const rxg_tcb_op *op)
{
    if (!c || !op) return fail(-EINVAL, "rxg_tcb_post: NULL argument");
    if (op->kind < RXG_TCB_OP_UPSERT || op->kind > RXG_TCB_OP_SET_STATE)
        return fail(-EINVAL, "rxg_tcb_post: kind %u", op->kind);
    if (!c->posted.push(*op)) return fail(-EAGAIN, "rxg_tcb_post: queue full (%u ops)", c->posted.capacity());
    return 0;
}

extern "C" int rxg_tcb_drain(rxg_ctx *c)
{
    if (!c) return fail(-EINVAL, "rxg_tcb_drain: ctx NULL");
    int applied = 0, first_err = 0;
    rxg_tcb_op op;
    while (c->posted.pop(op)) {
        int rc = 0;
        if (op.kind == RXG_TCB_OP_UPSERT) rc = rxg_tcb_upsert(c, op.idx, &op.tuple);
        else if (op.kind == RXG_TCB_OP_REMOVE) rc = rxg_tcb_remove(c, op.idx);
        else rc = rxg_tcb_set_state(c, op.idx, op.state);
        if (rc && !first_err) first_err = rc;
        ++applied;
    }
    return first_err ? first_err : applied;
}


// Burst boundary (rx thread): posted writes first, then the device mirror.
extern "C" int rxg_tcb_sync(rxg_ctx *c)
{
    if (!c) return fail(-EINVAL, "rxg_tcb_sync: ctx NULL");
    const int rc = rxg_tcb_drain(c);
    if (rc < 0) return rc;
    return tcb_push(c);
}

int tcb_push(rxg_ctx *c)
{
    if (!c->tables.tcb_stale()) return 0;
    if (int rc = set_device(c)) return rc;
    return c->tables.sync(&c->mir, nullptr, false);
}

// ------------------------------------------------- the tables' device side (HipTablePort) ---
int HipTablePort::event_create(Event *e, bool reader)
{
    // a reader's event, device-scope release: it orders streams of this device (and the host's
    // wait before a buffer is freed); no system-scope cache write-back
    HIP_OK(hipEventCreateWithFlags(e, hipEventDisableTiming | (reader ? hipEventReleaseToDevice : 0u)));
    return 0;
}

void HipTablePort::event_destroy(Event e) { (void)hipEventDestroy(e); }

int HipTablePort::record(Event e, Stream s) { HIP_OK(hipEventRecord(e, s)); return 0; }

int HipTablePort::stream_wait(Stream s, Event e) { HIP_OK(hipStreamWaitEvent(s, e, 0)); return 0; }

int HipTablePort::host_wait(Event e) { HIP_OK(hipEventSynchronize(e)); return 0; }

int HipTablePort::sync() { HIP_OK(hipStreamSynchronize(c->stream)); return 0; }

// device memory the host writes through a large BAR, else pinned host memory read over PCIe
int HipTablePort::patch_alloc(MirrorPatch **p, uint32_t cap, bool dev)
{
    const size_t bytes = (size_t)cap * sizeof(MirrorPatch);
    if (dev)
        HIP_OK(hipExtMallocWithFlags((void **)p, bytes, hipDeviceMallocFinegrained));
    else
        HIP_OK(hipHostMalloc((void **)p, bytes, hipHostMallocDefault));
    return 0;
}

int HipTablePort::patch_free(MirrorPatch *p, bool dev)
{
    HIP_OK(dev ? hipFree(p) : hipHostFree(p));
    return 0;
}

void HipTablePort::patch_write(MirrorPatch *dst, const MirrorPatch *src, uint32_t n, bool dev)
{
    std::memcpy(dst, src, (size_t)n * sizeof(MirrorPatch));
    if (dev) bar_publish(c, &dst[n - 1].v[3]);  // through the BAR: out before the launch
}

int HipTablePort::patch_launch(const MirrorPatch *list, uint32_t n, const DevBuf &buckets, const DevBuf &listen,
                               const DevBuf &arp)
{
    // the last replay's counter corrections ride along (its table writes are why this runs)
    CounterDelta d;
    if (c->pend) std::memcpy(d.v, c->pend_delta, sizeof d.v);
    HIP_OK(launch_mirror_patch(list, n, (uint4 *)buckets.p, (int32_t *)listen.p, (uint32_t *)arp.p, c->stream,
                               c->pend ? correction_row(c) : nullptr, &d));
    if (c->pend) {
        std::memset(c->pend_delta, 0, sizeof c->pend_delta);
        c->pend = false;
    }
    return 0;
}

int HipTablePort::table_resize(DevBuf &b, size_t bytes) { return ensure(b, bytes); }

int HipTablePort::table_upload(DevBuf &b, const void *src, size_t bytes)
{
    HIP_OK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// ----------------------------------------------------------------------- ARP mirror ---
extern "C" int rxg_arp_learned(rxg_ctx *c, uint32_t ip)
{
    if (!c) return fail(-EINVAL, "rxg_arp_learned: ctx NULL");
    c->arp_enabled = true;
    if (c->arp.add(ip)) c->tables.arp_changed();
    c->arp_since_burst.emplace(ip, 1);
    return 0;
}

extern "C" int rxg_arp_load(rxg_ctx *c, const uint32_t *ips, uint32_t n)
{
    if (!c || (n && !ips)) return fail(-EINVAL, "rxg_arp_load: bad arguments");
    c->arp_enabled = true;
    c->arp.clear();
    for (uint32_t i = 0; i < n; ++i) c->arp.add(ips[i]);
    c->tables.arp_changed();
    return 0;
}

extern "C" int32_t rxg_arp_count(rxg_ctx *c) { return c ? (int32_t)c->arp.ips.size() : -EINVAL; }

extern "C" int rxg_arp_disable(rxg_ctx *c)
{
    if (!c) return fail(-EINVAL, "rxg_arp_disable: ctx NULL");
    c->arp_enabled = false;
    c->arp.clear();
    c->arp_since_burst.clear();
    c->tables.arp_changed();
    return 0;
}

extern "C" int rxg_stream_register(rxg_ctx *c, void *stream)
{
    if (!c || !stream) return fail(-EINVAL, "rxg_stream_register: NULL argument");
    c->tables.register_stream((hipStream_t)stream);
    return 0;
}

extern "C" int rxg_stream_retire(rxg_ctx *c, void *stream)
{
    if (!c || !stream) return fail(-EINVAL, "rxg_stream_retire: NULL argument");
    if ((hipStream_t)stream == c->stream) return 0;
    if (int rc = set_device(c)) return rc;
    return c->tables.retire((hipStream_t)stream);
}

// ------------------------------------------------------------------------- bursts ---
void select_burst(rxg_ctx *c, uint32_t j)
{
    c->replay_cursor = j;
    const rxg_ctx::BurstRef &b = c->last_bursts[j];
    c->last_off = b.off64;
    c->last_slot0 = b.slot0;
    c->last_stride64 = b.stride64;
    c->last_len = b.len;
    c->last_n = b.n;
    c->last_recs = b.recs;
    c->pm.n = 0;  // a gather describes the burst it followed
}

int pm_handoff(rxg_ctx *c, hipStream_t st, const rxg_payload_msg *msgs, const uint64_t *used, uint32_t n)
{
    rxg_ctx::PayloadMsgs &pm = c->pm;
    if (!pm.ev) HIP_OK(hipEventCreateWithFlags(&pm.ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(pm.ev, st));
    pm.dev = msgs;
    pm.used = used;
    pm.n = n;
    pm.pending = true;  // rxg_payload_take fetches them on its first call after this one
    pm.poisoned = false;
    return 0;
}

// Validation, mirror sync and the replay bookkeeping of a burst set (launched or served).
// stride64 != 0: fixed-stride bursts (rxg_rx_bursts_strided_dev): bursts[j].off64 is unused and
// bursts[j].pad holds the burst's first slot.  carry: a launch on the context's stream follows
// and can take the mirrors' patch list (launch_bursts).
int begin_bursts(rxg_ctx *c, const void *frames, const rxg_dev_burst *bursts, uint32_t k, uint32_t rec_kind,
                 const char *who, uint32_t stride64, bool carry)
{
    // a rejected launch leaves nothing to replay: rxg_rx_replay refuses until a burst succeeds
    c->burst_ok = false;
    c->last_bursts.clear();
    if (!rec_kind_ok(rec_kind)) return fail(-EINVAL, "%s: rec_kind %u", who, rec_kind);
    if (k && !bursts) return fail(-EINVAL, "%s: NULL burst table", who);
    bool any = false;
    // the kernel reads descriptors as u32 / u16, frames in 16-byte chunks, and writes each
    // slice's records with 8- or 16-byte vector stores
    for (uint32_t j = 0; j < k; ++j) {
        if (!bursts[j].n) continue;
        if ((!stride64 && !bursts[j].off64) || !bursts[j].len || !bursts[j].out)
            return fail(-EINVAL, "%s: NULL device pointer in burst %u", who, j);
        if (stride64)
            if (int rc = check_frame_src(who, nullptr, bursts[j].pad, stride64, bursts[j].n, (int)j)) return rc;
        if (((uintptr_t)bursts[j].off64 & 3u) || ((uintptr_t)bursts[j].len & 1u) ||
            ((uintptr_t)bursts[j].out & (rec_align(rec_kind) - 1u)))
            return fail(-EINVAL, "%s: burst %u: off64 needs 4-byte, len 2-byte, out %u-byte alignment", who, j,
                        (unsigned)rec_align(rec_kind));
        any = true;
    }
    if (any && !frames) return fail(-EINVAL, "%s: NULL frame pool", who);
    if (any && ((uintptr_t)frames & 15u)) return fail(-EINVAL, "%s: frame pool not 16-byte aligned", who);
    int rc = set_device(c);
    if (rc) return rc;
    if ((rc = rxg_tcb_drain(c)) < 0) return rc;  // posted writes first, then the device tables
    if ((rc = c->tables.sync(&c->mir, c->arp_enabled ? &c->arp : nullptr, carry))) return rc;
    c->arp_since_burst.clear();
    c->last_frames = (const uint8_t *)frames;
    c->last_stride = rec_kind;
    for (uint32_t j = 0; j < k; ++j)
        c->last_bursts.push_back({stride64 ? nullptr : bursts[j].off64, bursts[j].len, bursts[j].n,
                                  (const uint8_t *)bursts[j].out, stride64 ? bursts[j].pad : 0u, stride64});
    if (c->last_bursts.empty()) c->last_bursts.push_back({nullptr, nullptr, 0u, nullptr});
    select_burst(c, 0);
    // the records reflect the mirror as of now: changes are tracked from here (replay)
    c->touched.clear();
    c->launch_writes.clear();
    return 0;
}

// Classify bursts[0..k) of one frame pool against the mirror as it stands: one launch per
// kMaxBursts bursts.  The bursts are then replayed in order (rxg_rx_replay).
static int launch_bursts(rxg_ctx *c, const void *frames, const rxg_dev_burst *bursts, uint32_t k, uint32_t rec_kind,
                         void *stream, const char *who, uint32_t stride64 = 0,
                         const rxg_payload_slots *pay = nullptr)
{
    hipStream_t st = pick(c, stream);
    // an unregistered stream is refused before anything changes (rxg.h: "-EINVAL, nothing
    // launched"): no mirror sync, and the previous burst stays replayable
    if (!c->tables.reader_allowed(st))
        return fail(-EINVAL, "%s: table-reading launch on stream %p, not registered with rxg_stream_register "
                             "(RXG_CFG_STREAMS_OUTLIVE_WRITES)", who, (void *)st);
    // The burst's first launch carries the mirror's patch list when nothing else reads the
    // tables meanwhile: launched on the context's stream (ordered after every earlier reader
    // there), no reader pending on another stream (TableSync::sync sees to that), and frames
    // in that launch (a launch of none is never made).  It then replaces a patch launch: ≈ 10 µs
    // of host launch latency per churning burst.
    bool first_has_frames = false;
    for (uint32_t j = 0; j < std::min(k, kMaxBursts); ++j) first_has_frames |= bursts[j].n != 0;
    int rc = begin_bursts(c, frames, bursts, k, rec_kind, who, stride64, st == c->stream && first_has_frames);
    if (rc) {
        (void)c->tables.abandon();
        return rc;
    }
    if ((rc = c->tables.before(st))) return rc;
    LaunchBurst lb[kMaxBursts];
    for (uint32_t j0 = 0; j0 < k; j0 += kMaxBursts) {
        const uint32_t m = std::min(kMaxBursts, k - j0);
        for (uint32_t j = 0; j < m; ++j)
            lb[j] = LaunchBurst{stride64 ? nullptr : bursts[j0 + j].off64, bursts[j0 + j].len, bursts[j0 + j].n,
                                (uint8_t *)bursts[j0 + j].out, stride64 ? bursts[j0 + j].pad : 0u};
        LaunchRx L;
        std::memset(&L, 0, sizeof L);
        L.frames = (const uint8_t *)frames;
        L.bursts = lb;
        L.nbursts = m;
        L.mode = (int)rec_kind;
        L.table = table_view(c);
        L.stride64 = stride64;
        if (pay) {
            L.pay_arena = (uint8_t *)pay->arena;
            L.pay_msgs = pay->msgs;
        }
        L.counters = c->counters;
        // (the by-reference hand-off writes no payload: its kernel's occupancy grid)
        L.max_blocks = pay && pay->arena ? grid_cap(c, c->op_grid[kGridPay]) : grid_for(c, rec_kind, pay != nullptr);
        L.ipatch = c->tables.carried(&L.nipatch);  // (the first launch takes it)
        const hipError_t e = launch_rx(L, st);
        if (e != hipSuccess) {
            (void)c->tables.abandon();
            HIP_OK(e);
        }
        if (L.nipatch && (rc = c->tables.carried_taken(st))) return rc;
    }
    if ((rc = c->tables.after(st))) return rc;
    c->burst_ok = true;
    // rxg_payload_take answers from this burst's messages (no look-back: never poisoned)
    if (pay && k == 1 && bursts[0].n) return pm_handoff(c, st, pay->msgs, nullptr, bursts[0].n);
    return 0;
}

extern "C" int rxg_rx_burst_dev(rxg_ctx *c, const rxg_dev_batch *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_rx_burst_dev: NULL argument");
    if (b->n && (!b->frames || !b->off64 || !b->len || !b->out))
        return fail(-EINVAL, "rxg_rx_burst_dev: NULL device pointer");
    const rxg_dev_burst one{b->off64, b->len, b->n, 0u, b->out};
    return launch_bursts(c, b->frames, &one, 1, b->rec_kind, stream, "rxg_rx_burst_dev");
}

static int check_slots(const rxg_payload_slots *p, uint32_t n, const char *who)
{
    if (n && !p->msgs) return fail(-EINVAL, "%s: NULL msgs", who);
    if ((uintptr_t)p->arena & 63u) return fail(-EINVAL, "%s: arena not 64-byte aligned", who);
    if ((uintptr_t)p->msgs & 15u) return fail(-EINVAL, "%s: msgs not 16-byte aligned", who);
    return 0;
}

extern "C" int rxg_rx_burst_payload_dev(rxg_ctx *c, const rxg_dev_batch *b, const rxg_payload_slots *p, void *stream)
{
    if (!c || !b || !p) return fail(-EINVAL, "rxg_rx_burst_payload_dev: NULL argument");
    if (b->n && (!b->frames || !b->off64 || !b->len || !b->out))
        return fail(-EINVAL, "rxg_rx_burst_payload_dev: NULL device pointer");
    if (int rc = check_slots(p, b->n, "rxg_rx_burst_payload_dev")) return rc;
    const rxg_dev_burst one{b->off64, b->len, b->n, 0u, b->out};
    return launch_bursts(c, b->frames, &one, 1, b->rec_kind, stream, "rxg_rx_burst_payload_dev", 0u, p);
}

extern "C" int rxg_rx_burst_strided_payload_dev(rxg_ctx *c, const void *frames, uint32_t stride64,
                                                const rxg_dev_strided_burst *b, uint32_t rec_kind,
                                                const rxg_payload_slots *p, void *stream)
{
    if (!c || !b || !p) return fail(-EINVAL, "rxg_rx_burst_strided_payload_dev: NULL argument");
    if (!stride64) return fail(-EINVAL, "rxg_rx_burst_strided_payload_dev: stride64 0");
    if (int rc = check_slots(p, b->n, "rxg_rx_burst_strided_payload_dev")) return rc;
    const rxg_dev_burst one{nullptr, b->len, b->n, b->slot0, b->out};
    return launch_bursts(c, frames, &one, 1, rec_kind, stream, "rxg_rx_burst_strided_payload_dev", stride64, p);
}

extern "C" int rxg_rx_bursts_dev(rxg_ctx *c, const void *frames, const rxg_dev_burst *bursts, uint32_t k,
                                 uint32_t rec_kind, void *stream)
{
    if (!c) return fail(-EINVAL, "rxg_rx_bursts_dev: ctx NULL");
    return launch_bursts(c, frames, bursts, k, rec_kind, stream, "rxg_rx_bursts_dev");
}

extern "C" int rxg_rx_bursts_strided_dev(rxg_ctx *c, const void *frames, uint32_t stride64,
                                         const rxg_dev_strided_burst *bursts, uint32_t k, uint32_t rec_kind,
                                         void *stream)
{
    if (!c) return fail(-EINVAL, "rxg_rx_bursts_strided_dev: ctx NULL");
    if (!stride64) return fail(-EINVAL, "rxg_rx_bursts_strided_dev: stride64 0");
    if (k && !bursts) return fail(-EINVAL, "rxg_rx_bursts_strided_dev: NULL burst table");
    std::vector<rxg_dev_burst> b(k);
    for (uint32_t j = 0; j < k; ++j) b[j] = rxg_dev_burst{nullptr, bursts[j].len, bursts[j].n, bursts[j].slot0, bursts[j].out};
    return launch_bursts(c, frames, b.data(), k, rec_kind, stream, "rxg_rx_bursts_strided_dev", stride64);
}

// The selected burst's offsets as a device array: its own off64, or for a fixed-stride burst
// slot0 + i * stride64 written into d_soff on `st` (the payload gather and the re-classify
// launch read offsets through a list; rare for strided bursts, which exist for the bulk path).
int burst_offsets(rxg_ctx *c, hipStream_t st, const uint32_t **out)
{
    *out = c->last_off;
    if (c->last_off || !c->last_stride64) return 0;
    // (rewritten for a reader on another stream: the same values, ordered on the reader's stream)
    if (c->soff_n != c->last_n || c->soff_slot0 != c->last_slot0 || c->soff_stride64 != c->last_stride64 ||
        c->soff_stream != st) {
        int rc = ensure(c->d_soff, (size_t)c->last_n * 4u);
        if (rc) return rc;
        HIP_OK(launch_strided_offsets((uint32_t *)c->d_soff.p, c->last_n, c->last_slot0, c->last_stride64, st));
        c->soff_n = c->last_n;
        c->soff_slot0 = c->last_slot0;
        c->soff_stride64 = c->last_stride64;
        c->soff_stream = st;
    }
    *out = (const uint32_t *)c->d_soff.p;
    return 0;
}

// ----------------------------------------------------------------------- counters ---
// The replay's counter corrections (rxg_rx_replay) wait on the host for the context's next
// mirror patch launch, which a replay that changed any record always leads to (the change
// came from a table write); a read, a sync or rxg_counters_dev adds them first.
int flush_delta(rxg_ctx *c)
{
    if (!c->pend) return 0;
    if (int rc = set_device(c)) return rc;
    CounterDelta d;
    std::memcpy(d.v, c->pend_delta, sizeof d.v);
    HIP_OK(launch_counters_add(correction_row(c), d, c->stream));
    std::memset(c->pend_delta, 0, sizeof c->pend_delta);
    c->pend = false;
    return 0;
}

extern "C" int rxg_counters_reset(rxg_ctx *c, void *stream)
{
    if (!c) return fail(-EINVAL, "rxg_counters_reset: ctx NULL");
    if (int rc = set_device(c)) return rc;
    // pending corrections belong to the bursts before the reset: zeroed with them
    std::memset(c->pend_delta, 0, sizeof c->pend_delta);
    c->pend = false;
    HIP_OK(hipMemsetAsync(c->counters, 0, kCounterBytes, pick(c, stream)));
    return 0;
}

extern "C" int rxg_counters_read(rxg_ctx *c, uint64_t *out)
{
    if (!c || !out) return fail(-EINVAL, "rxg_counters_read: NULL argument");
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_delta(c)) return rc;
    // bursts on caller streams add to the block too: every one launched so far is waited for
    // (the table readers' events), then the context's stream
    if (int rc = c->tables.wait_readers(true)) return rc;
    HIP_OK(hipStreamSynchronize(c->stream));
    std::vector<uint64_t> rows((size_t)RXG_COUNTER_ROWS * RXG_NCOUNTERS);
    HIP_OK(hipMemcpyAsync(rows.data(), c->counters, kCounterBytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < RXG_NCOUNTERS; ++k) {
        uint64_t v = 0;
        for (int r = 0; r < RXG_COUNTER_ROWS; ++r) v += rows[(size_t)r * RXG_NCOUNTERS + k];
        out[k] = v;
    }
    return 0;
}

extern "C" void *rxg_counters_dev(rxg_ctx *c)
{
    if (!c) return nullptr;
    (void)flush_delta(c);  // (on failure rxg_last_error says so; the block is still there)
    return (void *)c->counters;
}
