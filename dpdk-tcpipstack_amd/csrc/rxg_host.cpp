// rxg_host.cpp — host side of the rxg C ABI (include/rxg.h): the context, mirrors, launched
// bursts, tx and counters (the other entry points: rxg_server.cpp, rxg_replay.cpp,
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
        c->grid_pay = cus * 2u;
        c->grid_txb = cus * (uint32_t)tx_build_blocks_per_cu(false);  // rxg_tx_build_dev's occupancy grid
        c->grid_txbo = cus * (uint32_t)tx_build_blocks_per_cu(true);  // rxg_tx_build_opt_dev's
        c->grid_txr = cus * (uint32_t)tx_reset_blocks_per_cu();  // rxg_tx_reset_dev's
        c->grid_rxo = cus * (uint32_t)rx_opts_blocks_per_cu();  // rxg_rx_opts_dev's
        c->grid_txp = cus * (uint32_t)tx_plan_blocks_per_cu();  // rxg_tx_plan_dev's
        // rxg_flow_sums_dev's accumulation: one workgroup per CU.  Every workgroup ends with one
        // set of atomics on its carried flow, and atomics on one line run one after the other:
        // 256 workgroups measured faster than 1 024 on every shape
        c->grid_fs = cus;
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
                      &c->d_pg_ticket, &c->d_soff, &c->d_rst_counts, &c->d_txp_tiles, &c->d_fs_acc,
                      &c->d_fs_bits, &c->d_fs_tiles})
        if (b->p) (void)hipFree(b->p);
    if (c->rst_ev) (void)hipEventDestroy(c->rst_ev);
    if (c->txp_ev) (void)hipEventDestroy(c->txp_ev);
    if (c->fs_ev) (void)hipEventDestroy(c->fs_ev);
    if (c->h_pm) (void)hipHostFree(c->h_pm);
    if (c->pm_ev) (void)hipEventDestroy(c->pm_ev);
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
    if (tcb_key(t, k)) c->touched_keys.push_back(k);
    if (t.state == RXG_LISTENING && port_in_range(t.dport)) c->touched_listen.push_back(t.dport);
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
    if (c->mir.need_rebuild || c->mir.min_null != min_null) c->touched_pass2 = true;
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
    if (c->mir.need_rebuild || c->mir.min_null != min_null) c->touched_pass2 = true;
    if ((size_t)idx < c->rcv_state.size()) c->rcv_state[idx] = 0;  // FreeWindow
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
    c->touched_all = true;
    c->gen++;
    c->rcv_cur.clear();
    c->rcv_state.clear();
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
    c->touched_all = true;
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
    c->pm_n = 0;  // a gather describes the burst it followed
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
    const uintptr_t rec_align = rec_kind == RXG_REC8 ? 8u : 16u;
    for (uint32_t j = 0; j < k; ++j) {
        if (!bursts[j].n) continue;
        if ((!stride64 && !bursts[j].off64) || !bursts[j].len || !bursts[j].out)
            return fail(-EINVAL, "%s: NULL device pointer in burst %u", who, j);
        if (stride64 && (uint64_t)bursts[j].pad + (uint64_t)(bursts[j].n - 1u) * stride64 > 0xFFFFFFFFull)
            return fail(-EINVAL, "%s: burst %u: slot0 + (n - 1) * stride64 exceeds 2^32 - 1 slots", who, j);
        if (((uintptr_t)bursts[j].off64 & 3u) || ((uintptr_t)bursts[j].len & 1u) ||
            ((uintptr_t)bursts[j].out & (rec_align - 1u)))
            return fail(-EINVAL, "%s: burst %u: off64 needs 4-byte, len 2-byte, out %u-byte alignment", who, j,
                        (unsigned)rec_align);
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
    c->touched_keys.clear();
    c->touched_listen.clear();
    c->touched_all = c->touched_pass2 = false;
    c->launch_keys.clear();
    c->launch_listen.clear();
    c->launch_all = c->launch_pass2 = false;
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
        L.max_blocks = pay && pay->arena && !c->max_blocks ? c->grid_pay : grid_for(c, rec_kind, pay != nullptr);
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
    if (pay && k == 1 && bursts[0].n) {
        // rxg_payload_take answers from this burst's messages (fetched at its first call)
        if (!c->pm_ev) HIP_OK(hipEventCreateWithFlags(&c->pm_ev, hipEventDisableTiming));
        HIP_OK(hipEventRecord(c->pm_ev, st));
        c->d_pm = pay->msgs;
        c->pm_used = nullptr;  // no look-back: never poisoned
        c->pm_n = bursts[0].n;
        c->pm_pending = true;
        c->pm_poisoned = false;
    }
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

extern "C" int rxg_tx_cksum_dev(rxg_ctx *c, const rxg_dev_tx_batch *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_tx_cksum_dev: NULL argument");
    if (b->n && (!b->frames || !b->off64 || !b->len))
        return fail(-EINVAL, "rxg_tx_cksum_dev: NULL device pointer");
    if (b->n && (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u)))
        return fail(-EINVAL, "rxg_tx_cksum_dev: frames need 16-byte, off64 4-byte, len 2-byte alignment");
    int rc = set_device(c);
    if (rc) return rc;
    LaunchBurst one{b->off64, b->len, b->n, nullptr, 0u};
    LaunchRx L;
    std::memset(&L, 0, sizeof L);
    L.frames = (const uint8_t *)b->frames;
    L.bursts = &one;
    L.nbursts = 1;
    L.mode = 0;
    L.counters = nullptr;
    L.max_blocks = grid_for(c, 0);
    HIP_OK(launch_rx(L, pick(c, stream)));
    return 0;
}

static_assert(sizeof(rxg_tx_flow) == 32 && sizeof(rxg_tx_seg) == 32 && sizeof(rxg_dev_tx_build) == 80,
              "transmit segment build layouts");

// rxg_tx_build_dev and rxg_tx_build_opt_dev (`opt`: its block table): one argument check, one launch
static int tx_build_call(const char *who, rxg_ctx *c, const rxg_dev_tx_build *b, const rxg_dev_tx_build_opt *opt,
                         void *stream)
{
    if (!c || !b) return fail(-EINVAL, "%s: NULL argument", who);
    if (b->n == 0) return 0;
    if (!b->payload || !b->flows || !b->segs || !b->frames || !b->len)
        return fail(-EINVAL, "%s: NULL device pointer", who);
    if (((uintptr_t)b->payload & 15u) || ((uintptr_t)b->frames & 63u) || ((uintptr_t)b->segs & 7u) ||
        ((uintptr_t)b->flows & 7u) || ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u) ||
        ((uintptr_t)b->stats & 7u))
        return fail(-EINVAL, "%s: payload needs 16-byte, frames 64-byte, segs, flows and stats "
                             "8-byte, off64 4-byte, len 2-byte alignment", who);
    if (!b->off64) {
        if (!b->stride64) return fail(-EINVAL, "%s: stride64 0", who);
        if ((uint64_t)b->slot0 + (uint64_t)(b->n - 1u) * b->stride64 > 0xFFFFFFFFull)
            return fail(-EINVAL, "%s: slot0 + (n - 1) * stride64 exceeds 2^32 - 1 slots", who);
    }
    if (opt) {
        if ((uintptr_t)opt->opts & 15u) return fail(-EINVAL, "%s: opts needs 16-byte alignment", who);
        if (!opt->opts && opt->nopts) return fail(-EINVAL, "%s: NULL opts with nopts %u", who, opt->nopts);
    }
    int rc = set_device(c);
    if (rc) return rc;
    LaunchTxBuild L;
    L.payload = (const uint8_t *)b->payload;
    L.payload_bytes = b->payload_bytes;
    L.flows = b->flows;
    L.nflows = b->nflows;
    L.n = b->n;
    L.segs = b->segs;
    L.frames = (uint8_t *)b->frames;
    L.off64 = b->off64;
    L.slot0 = b->slot0;
    L.stride64 = b->stride64;
    L.len = b->len;
    L.stats = (unsigned long long *)b->stats;
    const uint32_t grid = opt ? c->grid_txbo : c->grid_txb;
    L.max_blocks = c->max_blocks ? c->max_blocks : (grid ? grid : 1024u);  // (as grid_for)
    L.with_opts = opt != nullptr;
    L.opts = opt ? opt->opts : nullptr;
    L.nopts = opt ? opt->nopts : 0u;
    HIP_OK(launch_tx_build(L, pick(c, stream)));
    return 0;
}

extern "C" int rxg_tx_build_dev(rxg_ctx *c, const rxg_dev_tx_build *b, void *stream)
{
    return tx_build_call("rxg_tx_build_dev", c, b, nullptr, stream);
}

static_assert(sizeof(rxg_tx_opt) == 48 && sizeof(rxg_dev_tx_build_opt) == 96, "option build layouts");

extern "C" int rxg_tx_build_opt_dev(rxg_ctx *c, const rxg_dev_tx_build_opt *b, void *stream)
{
    return tx_build_call("rxg_tx_build_opt_dev", c, b ? &b->b : nullptr, b, stream);
}

static_assert(sizeof(rxg_dev_tx_reset) == 88, "reset build layout");

extern "C" int rxg_tx_reset_dev(rxg_ctx *c, const rxg_dev_tx_reset *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_tx_reset_dev: NULL argument");
    if (!b->frames || !b->len || !b->recs || !b->out || !b->idx || !b->count)
        return fail(-EINVAL, "rxg_tx_reset_dev: NULL device pointer");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_tx_reset_dev: rec_kind %u", b->rec_kind);
    const uintptr_t rec_align = b->rec_kind == RXG_REC8 ? 8u : 16u;  // (as rxg_rx_burst_dev)
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->out & 63u) || ((uintptr_t)b->idx & 3u) ||
        ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u) || ((uintptr_t)b->count & 7u) ||
        ((uintptr_t)b->recs & (rec_align - 1u)))
        return fail(-EINVAL, "rxg_tx_reset_dev: frames need 16-byte, out 64-byte, idx and off64 4-byte, len 2-byte, "
                             "count 8-byte, recs %u-byte alignment", (unsigned)rec_align);
    if (!b->off64) {
        if (!b->stride64) return fail(-EINVAL, "rxg_tx_reset_dev: stride64 0");
        if (b->n && (uint64_t)b->slot0 + (uint64_t)(b->n - 1u) * b->stride64 > 0xFFFFFFFFull)
            return fail(-EINVAL, "rxg_tx_reset_dev: slot0 + (n - 1) * stride64 exceeds 2^32 - 1 slots");
    }
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = pick(c, stream);
    LaunchTxReset L;
    L.frames = (const uint8_t *)b->frames;
    L.off64 = b->off64;
    L.len = b->len;
    L.slot0 = b->slot0;
    L.stride64 = b->stride64;
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.out = (uint8_t *)b->out;
    L.idx = b->idx;
    L.cap = b->cap;
    L.count = (unsigned long long *)b->count;
    L.counts = nullptr;
    L.ip_id0 = b->ip_id0;
    std::memcpy(L.src_mac, b->src_mac, 6);
    L.max_blocks = c->max_blocks ? c->max_blocks : (c->grid_txr ? c->grid_txr : 1024u);  // (as grid_for)
    if (b->n) {
        // One call at a time uses the context's slice counts: a call waits, on its stream, for
        // the previous call's last launch (rst_ev); before the buffer is replaced for a larger
        // n the host waits for that launch instead.
        const size_t need = tx_reset_count_bytes(b->n);
        if (c->rst_ev && c->d_rst_counts.bytes < need) HIP_OK(hipEventSynchronize(c->rst_ev));
        if ((rc = ensure(c->d_rst_counts, need))) return rc;
        if (c->rst_ev) HIP_OK(hipStreamWaitEvent(st, c->rst_ev, 0));
        else HIP_OK(hipEventCreateWithFlags(&c->rst_ev, hipEventDisableTiming));
        L.counts = (uint32_t *)c->d_rst_counts.p;
    }
    const hipError_t e = launch_tx_reset(L, st);
    // (recorded even after a failed launch: whatever part of it was enqueued is waited for)
    if (b->n) HIP_OK(hipEventRecord(c->rst_ev, st));
    HIP_OK(e);
    return 0;
}

static_assert(sizeof(rxg_tx_send) == 40 && sizeof(rxg_dev_tx_plan) == 80, "device planner layouts");

extern "C" int rxg_tx_plan_dev(rxg_ctx *c, const rxg_dev_tx_plan *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_tx_plan_dev: NULL argument");
    if (!b->sends || !b->first || !b->count || (!b->segs && b->cap))
        return fail(-EINVAL, "rxg_tx_plan_dev: NULL device pointer");
    if (((uintptr_t)b->sends & 7u) || ((uintptr_t)b->segs & 7u) || ((uintptr_t)b->first & 7u) ||
        ((uintptr_t)b->count & 7u) || ((uintptr_t)b->opts & 15u) || ((uintptr_t)b->next_seq & 3u) ||
        ((uintptr_t)b->send_opt & 3u))
        return fail(-EINVAL, "rxg_tx_plan_dev: sends, segs, first and count need 8-byte, opts 16-byte, next_seq and "
                             "send_opt 4-byte alignment");
    if (b->mss == 0 || b->mss > RXG_TX_MAX_DATA) return fail(-EINVAL, "rxg_tx_plan_dev: mss %u", b->mss);
    if (!b->opts && b->nopts) return fail(-EINVAL, "rxg_tx_plan_dev: NULL opts with nopts %u", b->nopts);
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = pick(c, stream);
    LaunchTxPlan L;
    L.sends = b->sends;
    L.nsends = b->nsends;
    L.mss = b->mss;
    L.send_opt = b->send_opt;
    L.opts = b->opts;
    L.nopts = b->nopts;
    L.segs = b->segs;
    L.cap = b->cap;
    L.first = (unsigned long long *)b->first;
    L.next_seq = b->next_seq;
    L.count = (unsigned long long *)b->count;
    L.tiles = nullptr;
    L.max_blocks = c->max_blocks ? c->max_blocks : (c->grid_txp ? c->grid_txp : 1024u);  // (as grid_for)
    if (b->nsends) {
        // One call at a time uses the context's tile sums (rxg_tx_reset_dev's rule): a call
        // waits, on its stream, for the previous call's last launch (txp_ev); before the buffer
        // is replaced for more sends the host waits for that launch instead.
        const size_t need = tx_plan_tile_bytes(b->nsends);
        if (c->txp_ev && c->d_txp_tiles.bytes < need) HIP_OK(hipEventSynchronize(c->txp_ev));
        if ((rc = ensure(c->d_txp_tiles, need))) return rc;
        if (c->txp_ev) HIP_OK(hipStreamWaitEvent(st, c->txp_ev, 0));
        else HIP_OK(hipEventCreateWithFlags(&c->txp_ev, hipEventDisableTiming));
        L.tiles = c->d_txp_tiles.p;
    }
    const hipError_t e = launch_tx_plan(L, st);
    // (recorded even after a failed launch: whatever part of it was enqueued is waited for)
    if (b->nsends) HIP_OK(hipEventRecord(c->txp_ev, st));
    HIP_OK(e);
    return 0;
}

static_assert(sizeof(rxg_rx_opt) == 16 && sizeof(rxg_dev_rx_opts) == 56, "received-option layouts");

extern "C" int rxg_rx_opts_dev(rxg_ctx *c, const rxg_dev_rx_opts *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_rx_opts_dev: NULL argument");
    if (!b->frames || !b->len || !b->recs || !b->out) return fail(-EINVAL, "rxg_rx_opts_dev: NULL device pointer");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_rx_opts_dev: rec_kind %u", b->rec_kind);
    const uintptr_t rec_align = b->rec_kind == RXG_REC8 ? 8u : 16u;  // (as rxg_rx_burst_dev)
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->out & 15u) || ((uintptr_t)b->off64 & 3u) ||
        ((uintptr_t)b->len & 1u) || ((uintptr_t)b->recs & (rec_align - 1u)))
        return fail(-EINVAL, "rxg_rx_opts_dev: frames and out need 16-byte, off64 4-byte, len 2-byte, recs %u-byte "
                             "alignment", (unsigned)rec_align);
    if (!b->off64) {
        if (!b->stride64) return fail(-EINVAL, "rxg_rx_opts_dev: stride64 0");
        if (b->n && (uint64_t)b->slot0 + (uint64_t)(b->n - 1u) * b->stride64 > 0xFFFFFFFFull)
            return fail(-EINVAL, "rxg_rx_opts_dev: slot0 + (n - 1) * stride64 exceeds 2^32 - 1 slots");
    }
    if (!b->n) return 0;
    int rc = set_device(c);
    if (rc) return rc;
    LaunchRxOpts L;
    L.frames = (const uint8_t *)b->frames;
    L.off64 = b->off64;
    L.len = b->len;
    L.slot0 = b->slot0;
    L.stride64 = b->stride64;
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.out = (uint8_t *)b->out;
    L.max_blocks = c->max_blocks ? c->max_blocks : (c->grid_rxo ? c->grid_rxo : 1024u);  // (as grid_for)
    HIP_OK(launch_rx_opts(L, pick(c, stream)));
    return 0;
}

static_assert(sizeof(rxg_flow_sum) == 40 && sizeof(rxg_dev_flow_sums) == 80, "flow summary layouts");

// b grown to `bytes` (never shrunk) for rxg_flow_sums_dev.  zero: the new memory is zeroed on
// st -- the old held nothing but zeroes once the previous call was done, which the host waits
// for before the buffer is replaced.  -ENOMEM when it cannot be had (b is then empty).
static int fs_grow(rxg_ctx *c, DevBuf &b, size_t bytes, bool zero, hipStream_t st)
{
    if (b.p && b.bytes >= bytes) return 0;
    if (c->fs_ev) HIP_OK(hipEventSynchronize(c->fs_ev));
    if (b.p) HIP_OK(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    const size_t want = std::max<size_t>(bytes, 256);
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(-ENOMEM, "rxg_flow_sums_dev: %zu bytes of device memory", want);
    }
    b.bytes = want;
    if (zero) HIP_OK(hipMemsetAsync(b.p, 0, want, st));
    return 0;
}

extern "C" int rxg_flow_sums_dev(rxg_ctx *c, const rxg_dev_flow_sums *b, void *stream)
{
    if (!c || !b) return fail(-EINVAL, "rxg_flow_sums_dev: NULL argument");
    if (!rec_kind_ok(b->rec_kind)) return fail(-EINVAL, "rxg_flow_sums_dev: rec_kind %u", b->rec_kind);
    const bool reads_frames = b->rec_kind != RXG_REC48;
    if (!b->recs || !b->count || (!b->out && b->cap) || (reads_frames && (!b->frames || !b->len)))
        return fail(-EINVAL, "rxg_flow_sums_dev: NULL device pointer");
    if (b->ntcb == 0 || b->ntcb > RXG_FS_MAX_NTCB) return fail(-EINVAL, "rxg_flow_sums_dev: ntcb %u", b->ntcb);
    if (b->flags & ~RXG_FS_TCP_OK_ONLY) return fail(-EINVAL, "rxg_flow_sums_dev: unknown flags 0x%x", b->flags);
    const uintptr_t rec_align = b->rec_kind == RXG_REC8 ? 8u : 16u;  // (as rxg_rx_burst_dev)
    if (((uintptr_t)b->frames & 15u) || ((uintptr_t)b->out & 7u) || ((uintptr_t)b->count & 7u) ||
        ((uintptr_t)b->off64 & 3u) || ((uintptr_t)b->len & 1u) || ((uintptr_t)b->recs & (rec_align - 1u)))
        return fail(-EINVAL, "rxg_flow_sums_dev: frames need 16-byte, out and count 8-byte, off64 4-byte, len 2-byte, "
                             "recs %u-byte alignment", (unsigned)rec_align);
    if (reads_frames && !b->off64) {
        if (!b->stride64) return fail(-EINVAL, "rxg_flow_sums_dev: stride64 0");
        if (b->n && (uint64_t)b->slot0 + (uint64_t)(b->n - 1u) * b->stride64 > 0xFFFFFFFFull)
            return fail(-EINVAL, "rxg_flow_sums_dev: slot0 + (n - 1) * stride64 exceeds 2^32 - 1 slots");
    }
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = pick(c, stream);
    LaunchFlowSum L;
    L.frames = reads_frames ? (const uint8_t *)b->frames : nullptr;
    L.off64 = b->off64;
    L.len = b->len;
    L.slot0 = b->slot0;
    L.stride64 = b->stride64;
    L.n = b->n;
    L.rec_kind = b->rec_kind;
    L.recs = (const uint8_t *)b->recs;
    L.ntcb = b->ntcb;
    L.flags = b->flags;
    L.out = b->out;
    L.cap = b->cap;
    L.count = (unsigned long long *)b->count;
    L.acc = nullptr;
    L.bits = nullptr;
    L.tiles = nullptr;
    L.max_blocks = c->max_blocks;
    L.acc_blocks = c->grid_fs ? c->grid_fs : 1024u;
    if (b->n) {
        // One call at a time uses the context's accumulator, bitmap and tile counts
        // (rxg_tx_reset_dev's rule): a call waits, on its stream, for the previous call's last
        // launch (fs_ev); before a buffer is replaced for a larger ntcb the host waits instead.
        if ((rc = fs_grow(c, c->d_fs_acc, flow_sum_bytes(b->ntcb), true, st))) return rc;
        if ((rc = fs_grow(c, c->d_fs_bits, flow_sum_bits_bytes(b->ntcb), true, st))) return rc;
        if ((rc = fs_grow(c, c->d_fs_tiles, flow_sum_tile_bytes(b->ntcb), false, st))) return rc;
        if (c->fs_ev) HIP_OK(hipStreamWaitEvent(st, c->fs_ev, 0));
        else HIP_OK(hipEventCreateWithFlags(&c->fs_ev, hipEventDisableTiming));
        if (c->fs_dirty) {
            HIP_OK(hipMemsetAsync(c->d_fs_acc.p, 0, c->d_fs_acc.bytes, st));
            HIP_OK(hipMemsetAsync(c->d_fs_bits.p, 0, c->d_fs_bits.bytes, st));
            c->fs_dirty = false;
        }
        L.acc = (FlowSumAcc *)c->d_fs_acc.p;
        L.bits = (uint32_t *)c->d_fs_bits.p;
        L.tiles = (uint32_t *)c->d_fs_tiles.p;
    }
    const hipError_t e = launch_flow_sum(L, st);
    if (b->n && e != hipSuccess) c->fs_dirty = true;
    // (recorded even after a failed launch: whatever part of it was enqueued is waited for)
    if (b->n) HIP_OK(hipEventRecord(c->fs_ev, st));
    HIP_OK(e);
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
