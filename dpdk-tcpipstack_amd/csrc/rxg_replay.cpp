// rxg_replay.cpp — the per-packet replay of a classified burst into the caller's handlers
// (rxg_rx_replay: the reference's ether_in -> ip_in -> tcp_in order, re-classifying what a
// handler's table write changed), the payload hand-off (rxg_payload_gather_dev, rxg_rcv_set,
// rxg_payload_take), the C entry points of what a replay hands out (resets, options, flow
// summaries, flow trains, ACKs: their rules are rxg_attached.h's) and the one-frame rxg_ether_in.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstring>
#include <immintrin.h>
#include <thread>

#include "rxg_ctx.h"

using namespace rxg;

extern "C" int rxg_ether_in(rxg_ctx *c, const rxg_handoff_ops *ops, void *mbuf, void *frame, uint16_t data_len)
{
    if (!c || !ops || !frame) return fail(-EINVAL, "rxg_ether_in: NULL argument");
    rxg_pkt_view v;
    v.buf_addr = frame;
    v.data_off = 0;
    v.data_len = data_len;
    v.pad = 0;
    rxg_rec16 rec;
    int rc = rxg_rx_burst(c, &v, 1, RXG_REC16, &rec);
    if (rc) return rc;
    void *m = mbuf, *f = frame;
    rc = rxg_rx_replay(c, ops, &m, &f, &rec, 1, RXG_REC16);
    return rc ? rc : 0;  // ether_in always returns 0 (etherin.c:36)
}

// ----------------------------------------------------------------- payload hand-off ---
extern "C" int rxg_payload_gather_dev(rxg_ctx *c, const rxg_payload_out *o, void *stream)
{
    if (!c || !o) return fail(-EINVAL, "rxg_payload_gather_dev: NULL argument");
    if (!c->last_frames || !c->last_recs)
        return fail(-EINVAL, "rxg_payload_gather_dev: no burst to gather from");
    const uint32_t n = c->last_n;
    if (n && (!o->msgs || !o->arena_used || (o->arena_cap && !o->arena)))
        return fail(-EINVAL, "rxg_payload_gather_dev: NULL output buffer");
    int rc = set_device(c);
    if (rc) return rc;
    hipStream_t st = pick(c, stream);
    const uint32_t nb = payload_blocks(n);
    const void *old_status = c->d_pg_status.p;
    if ((rc = ensure(c->d_pg_status, (size_t)nb * sizeof(unsigned long long)))) return rc;
    if (c->d_pg_status.p != old_status)  // fresh memory: no word may look published
        HIP_OK(hipMemsetAsync(c->d_pg_status.p, 0, c->d_pg_status.bytes, st));
    if (!c->d_pg_ticket.p) {
        if ((rc = ensure(c->d_pg_ticket, sizeof(unsigned long long)))) return rc;
        HIP_OK(hipMemsetAsync(c->d_pg_ticket.p, 0, sizeof(unsigned long long), st));
        c->pg_tickets = 0;
    }
    // one gather in flight per context: the ticket counter and the status words are shared,
    // so a gather on another stream waits for the previous one
    if (c->pm.ev) HIP_OK(hipStreamWaitEvent(st, c->pm.ev, 0));
    c->pg_epoch = (c->pg_epoch % ((1u << 30) - 1u)) + 1u;
    LaunchPayload P;
    P.frames = c->last_frames;
    if ((rc = burst_offsets(c, st, &P.off64))) return rc;
    P.len = c->last_len;
    P.recs = c->last_recs;
    P.stride = c->last_stride;
    P.n = n;
    P.msgs = o->msgs;
    P.arena = (uint8_t *)o->arena;
    P.arena_cap = o->arena ? o->arena_cap : 0;
    P.status = (unsigned long long *)c->d_pg_status.p;
    P.ticket = (unsigned long long *)c->d_pg_ticket.p;
    P.ticket_base = c->pg_tickets;
    P.used = (unsigned long long *)o->arena_used;
    P.epoch = c->pg_epoch;
    uint32_t tickets = 0;
    HIP_OK(launch_payload(P, st, &tickets));
    c->pg_tickets += tickets;
    return pm_handoff(c, st, o->msgs, o->arena_used, n);
}

extern "C" int rxg_rcv_set(rxg_ctx *c, int32_t idx, uint32_t cur_seq, uint32_t pairs_pending)
{
    if (!c) return fail(-EINVAL, "rxg_rcv_set: ctx NULL");
    if (idx < 0 || idx >= kMaxTcbs) return fail(-EINVAL, "rxg_rcv_set: index %d", idx);
    c->rcv.set(idx, cur_seq, pairs_pending != 0);
    return 0;
}

// The messages of the last gather into the pinned host copy, and whether its look-back timed out.
static int pm_fetch(rxg_ctx *c)
{
    rxg_ctx::PayloadMsgs &pm = c->pm;
    if (int rc = set_device(c)) return rc;
    HIP_OK(hipEventSynchronize(pm.ev));
    if (pm.n > pm.host_cap) {
        if (pm.host) HIP_OK(hipHostFree(pm.host));
        pm.host = nullptr;
        pm.host_cap = 0;
        HIP_OK(hipHostMalloc((void **)&pm.host, (size_t)pm.n * sizeof(rxg_payload_msg), hipHostMallocDefault));
        pm.host_cap = pm.n;
    }
    uint64_t used = 0;
    HIP_OK(hipMemcpyAsync(pm.host, pm.dev, (size_t)pm.n * sizeof(rxg_payload_msg), hipMemcpyDeviceToHost, c->stream));
    if (pm.used)  // (a fused burst, rxg_rx_burst_payload_dev, has no look-back to time out)
        HIP_OK(hipMemcpyAsync(&used, pm.used, sizeof used, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    pm.pending = false;
    // a gather whose look-back timed out (arena_used = ~0) placed payloads at unknown
    // offsets: nothing of that burst is handed out (the stack's own PushData runs)
    pm.poisoned = used == ~0ull;
    return 0;
}

// The message of the packet being replayed, if the window of tcbs[idx] takes it (RcvWindow::take).
extern "C" int rxg_payload_take(rxg_ctx *c, int32_t idx, uint32_t seq, uint32_t length, rxg_payload_msg *msg)
{
    if (!c) return fail(-EINVAL, "rxg_payload_take: ctx NULL");
    const int64_t pos = c->attached.position();
    if (pos < 0 || (uint64_t)pos >= c->pm.n || length == 0 || length > 0xFFFFu) return 0;
    if (c->pm.pending)  // first take after the gather
        if (int rc = pm_fetch(c)) return rc;
    if (c->pm.poisoned) return 0;
    const rxg_payload_msg &m = c->pm.host[pos];
    if (!c->rcv.take(idx, seq, length, m)) return 0;
    if (msg) *msg = m;
    return 1;
}

// ---------------------------------------------------- what a replay hands out ---
// (the rules: rxg::ReplayAttached, rxg_attached.h)
extern "C" int rxg_reset_attach(rxg_ctx *c, void *resets_host, const uint32_t *idx_host, uint64_t nbuilt)
{
    if (!c || (nbuilt && (!resets_host || !idx_host)))
        return fail(-EINVAL, "rxg_reset_attach: NULL argument");
    c->attached.attach_resets(resets_host, idx_host, nbuilt);
    return 0;
}

extern "C" int rxg_reset_take(rxg_ctx *c, uint16_t ip_id, void **frame_out)
{
    if (!c || !frame_out) return fail(-EINVAL, "rxg_reset_take: NULL argument");
    uint8_t *f = c->attached.take_reset(ip_id);
    if (!f) return 0;
    *frame_out = f;
    return 1;
}

extern "C" int rxg_rx_opts_attach(rxg_ctx *c, const rxg_rx_opt *opts_host, uint32_t n)
{
    if (!c || (n && !opts_host)) return fail(-EINVAL, "rxg_rx_opts_attach: NULL argument");
    c->attached.attach_opts(opts_host, n);
    return 0;
}

extern "C" int rxg_rx_opt_current(rxg_ctx *c, const rxg_rx_opt **out)
{
    if (!c || !out) return fail(-EINVAL, "rxg_rx_opt_current: NULL argument");
    const rxg_rx_opt *o = c->attached.opt_current();
    if (!o) return 0;
    *out = o;
    return 1;
}

extern "C" int rxg_flow_sums_attach(rxg_ctx *c, const rxg_flow_sum *sums_host, uint64_t m)
{
    if (!c || (m && !sums_host)) return fail(-EINVAL, "rxg_flow_sums_attach: NULL argument");
    uint64_t k = 0;
    if (!c->attached.attach_flow_sums(sums_host, m, &k))
        return fail(-EINVAL, "rxg_flow_sums_attach: entry %llu is not above its predecessor's tcb_idx",
                    (unsigned long long)k);
    return 0;
}

extern "C" int rxg_flow_sum_current(rxg_ctx *c, const rxg_flow_sum **out, uint32_t *pkt_idx)
{
    if (!c || !out || !pkt_idx) return fail(-EINVAL, "rxg_flow_sum_current: NULL argument");
    const rxg_flow_sum *s = c->attached.flow_sum_current(c->replay, pkt_idx);
    if (!s) return 0;
    *out = s;
    return 1;
}

extern "C" int rxg_flow_trains_attach(rxg_ctx *c, const uint32_t *order_host, uint64_t nseg,
                                      const rxg_flow_train *trains_host, uint64_t ntrains)
{
    if (!c || (nseg && !order_host) || (ntrains && !trains_host))
        return fail(-EINVAL, "rxg_flow_trains_attach: NULL argument");
    uint64_t k = 0, first = 0;
    if (!c->attached.attach_flow_trains(order_host, nseg, trains_host, ntrains, &k, &first))
        return fail(-EINVAL, "rxg_flow_trains_attach: train %llu does not start where its predecessor ended "
                             "(first %u, nseg %u, expected first %llu)",
                    (unsigned long long)k, trains_host[k].first, trains_host[k].nseg, (unsigned long long)first);
    return 0;
}

extern "C" int rxg_flow_train_current(rxg_ctx *c, const rxg_flow_train **out, uint32_t *pos_out)
{
    if (!c || !out || !pos_out) return fail(-EINVAL, "rxg_flow_train_current: NULL argument");
    const rxg_flow_train *t = c->attached.flow_train_current(c->replay, pos_out);
    if (!t) return 0;
    *out = t;
    return 1;
}

extern "C" int rxg_acks_attach(rxg_ctx *c, const rxg_ack *acks_host, void *frames_host, uint32_t stride, uint64_t nacks)
{
    if (!c || (nacks && (!acks_host || !frames_host || !stride)))
        return fail(-EINVAL, "rxg_acks_attach: NULL argument or stride 0");
    uint64_t a = 0;
    if (!c->attached.attach_acks(acks_host, frames_host, stride, nacks, &a))
        return fail(-EINVAL, "rxg_acks_attach: entry %llu is not above its predecessor's tcb_idx",
                    (unsigned long long)a);
    return 0;
}

// (rxg_ctx::touched: the writes no replay has absorbed yet, kept until the next burst)
extern "C" int rxg_ack_take(rxg_ctx *c, int32_t tcb_idx, uint32_t snd_nxt, uint32_t rcv_ack, void **frame_out)
{
    if (!c || !frame_out) return fail(-EINVAL, "rxg_ack_take: NULL argument");
    uint8_t *f = c->attached.ack_take(tcb_idx, snd_nxt, rcv_ack, c->mir, c->touched);
    if (!f) return 0;
    *frame_out = f;
    return 1;
}

// ------------------------------------------------------------------------- replay ---
// Counter contributions of one TCP record (the kernel's definition; only the fields a
// re-classification can change).
static void tcp_record_counters(const rxg_rec16 &r, int64_t sign, int64_t *d)
{
    if (r.flags & RXG_F_REF_NULLSLOT) d[RXG_C_REF_NULLSLOT] += sign;
    if (r.tcb_idx >= 0) d[(r.flags & RXG_F_LISTEN) ? RXG_C_TCB_HIT_LISTEN : RXG_C_TCB_HIT_EXACT] += sign;
    if (r.verdict == RXG_V_RST_NOPCB) d[RXG_C_NOPCB] += sign;
    if (r.verdict == RXG_V_RST_LISTEN_NONSYN) d[RXG_C_LISTEN_NONSYN] += sign;
    if (r.verdict == RXG_V_DISPATCH) d[RXG_C_DISPATCH] += sign;
}

// Re-classify one TCP packet of >= 54 bytes against the table as it stands now, exactly as
// rx_kernel's classify does (findtcb tcp_tcb.c:127-173, tcp_in.c:47-59), answered from the
// host index the device mirror is patched from (rxg_mirror.h): the replay's fix-up of a
// packet whose TCB a handler changed inside the burst.  The fields a
// table change cannot move (checksums, datalen, flags of the frame) stay as the burst
// computed them.
static void host_classify(const TcbMirror &mir, const uint8_t *f, rxg_rec16 &r)
{
    const TupleKey k = frame_key(f);
    uint8_t st = RXG_STATE_NONE;
    bool lhit = false;
    const int32_t idx = mir.find(k.ports, k.dst, k.src, k.ports >> 16, &st, &lhit);
    const bool missed = idx < 0 || lhit;  // pass 1 found nothing
    const bool nslot = missed && mir.min_null < (lhit ? idx : mir.ntcb());
    const uint8_t tflags = f[47];
    r.tcb_idx = idx;
    r.state = idx >= 0 ? st : (uint8_t)RXG_STATE_NONE;
    r.verdict = idx < 0 ? RXG_V_RST_NOPCB
              : (st == RXG_LISTENING && !(tflags & RXG_TCP_FLAG_SYN)) ? RXG_V_RST_LISTEN_NONSYN
              : RXG_V_DISPATCH;
    r.flags = (uint8_t)((r.flags & ~(RXG_F_LISTEN | RXG_F_REF_NULLSLOT)) | (lhit ? RXG_F_LISTEN : 0) |
                        (nslot ? RXG_F_REF_NULLSLOT : 0));
}

// Re-classify frames sel[0..k) of the last burst against the current mirror (GPU).
static int reclassify(rxg_ctx *c, const std::vector<uint32_t> &sel, std::vector<rxg_rec16> &out)
{
    int rc;
    const uint32_t *off64 = nullptr;
    if ((rc = burst_offsets(c, c->stream, &off64))) return rc;
    if (!c->last_frames || !off64 || !c->last_len)
        return fail(-EINVAL, "rxg_rx_replay: no burst on this context to re-classify against");
    if ((rc = ensure(c->d_sel, sel.size() * 4))) return rc;
    if ((rc = ensure(c->d_fix, sel.size() * sizeof(rxg_rec16)))) return rc;
    if ((rc = tcb_push(c))) return rc;
    HIP_OK(hipMemcpyAsync(c->d_sel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, c->stream));
    const LaunchBurst one{off64, c->last_len, (uint32_t)sel.size(), (uint8_t *)c->d_fix.p, 0u};
    LaunchRx L;
    std::memset(&L, 0, sizeof L);
    L.frames = c->last_frames;
    L.bursts = &one;
    L.nbursts = 1;
    L.sel = (const uint32_t *)c->d_sel.p;
    L.mode = RXG_REC16;
    L.table = table_view(c);
    L.counters = nullptr;  // corrections go to the host row instead
    L.max_blocks = grid_for(c, RXG_REC16);
    HIP_OK(launch_rx(L, c->stream));
    out.resize(sel.size());
    HIP_OK(hipMemcpyAsync(out.data(), c->d_fix.p, sel.size() * sizeof(rxg_rec16), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

// One batch of table writes into the replay's log, and to what the replay hands out.
static void absorb(rxg_ctx *c, const WriteSet &w)
{
    c->attached.wrote(w);
    c->replay.absorb(w);
}

// The tracked writes since the last absorb; logged for the launch's later bursts, whose records
// were computed before them too.
static void absorb_touched(rxg_ctx *c)
{
    c->launch_writes.add(c->touched);
    absorb(c, c->touched);
    c->touched.clear();
}

// Packet j's record becomes r: the counter corrections, and what the replay hands out told.
static void refix(rxg_ctx *c, uint32_t j, const rxg_rec16 &r, int64_t *delta)
{
    const rxg_rec16 &old = c->replay.record(j);
    tcp_record_counters(old, -1, delta);
    tcp_record_counters(r, +1, delta);
    c->attached.refixed(old, r);
    c->replay.fixed(j, r);
}

// The side effects of etherin.c:21-35, ip.c:26-39 and tcp_in.c:47-72 for one packet.
static void dispatch(rxg_ctx *c, const rxg_handoff_ops *ops, const rxg_rec16 &r, void *m, uint8_t *f)
{
    void *ip = f + RXG_OFF_IP, *tcp = f + RXG_OFF_TCP;
    switch (r.verdict) {
    case RXG_V_ARP:
        if (ops->arp_in) ops->arp_in(ops->user, m);
        if (ops->free_mbuf) ops->free_mbuf(ops->user, m);
        break;
    case RXG_V_DROP_L2:
    case RXG_V_DROP_NONTCP:
        if (ops->free_mbuf) ops->free_mbuf(ops->user, m);
        break;
    default: {
        // ip.c:30-32 ARP learn on the host-order source address
        const uint32_t src = ((uint32_t)f[26] << 24) | ((uint32_t)f[27] << 16) | ((uint32_t)f[28] << 8) | f[29];
        if (c->arp_enabled) {
            // the mirror answers get_mac: unknown at the burst and not added since
            if ((r.flags & RXG_F_ARP_LEARN) && ops->add_mac && !c->arp_since_burst.count(src)) {
                ops->add_mac(ops->user, src, f + 6);
                rxg_arp_learned(c, src);  // idempotent if the caller's add_mac mirrors too
            }
        } else {
            unsigned char mac[6];
            if (ops->get_mac && ops->add_mac && ops->get_mac(ops->user, src, mac) == 0)
                ops->add_mac(ops->user, src, f + 6);
        }
        if ((ops->flags & RXG_OPS_VERIFY_TCP_CKSUM) && !(r.flags & RXG_F_TCP_OK)) {
            // tcp_in.c:37-40 with the check compiled in: free, ++tcpchecksumerror
            if (ops->free_mbuf) ops->free_mbuf(ops->user, m);
            if (ops->tcpchecksumerror) ++*ops->tcpchecksumerror;
        } else if (r.verdict == RXG_V_RST_NOPCB || r.verdict == RXG_V_RST_LISTEN_NONSYN) {
            if (r.verdict == RXG_V_RST_NOPCB && ops->tcpnopcb) ++*ops->tcpnopcb;  // tcp_in.c:48
            if (ops->free_mbuf) ops->free_mbuf(ops->user, m);
            if (ops->send_reset) ops->send_reset(ops->user, ip, tcp);
        } else {  // RXG_V_DISPATCH
            const uint32_t seq = ((uint32_t)f[38] << 24) | ((uint32_t)f[39] << 16) | ((uint32_t)f[40] << 8) | f[41];
            const uint32_t ack = ((uint32_t)f[42] << 24) | ((uint32_t)f[43] << 16) | ((uint32_t)f[44] << 8) | f[45];
            if (ops->on_segment) ops->on_segment(ops->user, r.tcb_idx, seq, ack);
            if (ops->tcpswitch) ops->tcpswitch(ops->user, r.tcb_idx, r.state, tcp, ip, m);
        }
    }
    }
}

// The burst's packets into the caller's handlers in packet order; a packet whose record a table
// write made stale (rxg::ReplayLog, rxg_replaylog.h) is re-classified before its handlers run.
extern "C" int rxg_rx_replay(rxg_ctx *c, const rxg_handoff_ops *ops, void *const *mbufs,
                             void *const *frames, const void *recs, uint32_t n, uint32_t stride)
{
    if (!c) return fail(-EINVAL, "rxg_rx_replay: NULL argument");
    ReplayAttached &att = c->attached;
    // on every way out, a failed argument check included
    struct Ending {
        ReplayAttached &a;
        bool ran_to_end = false;
        ~Ending() { a.end_replay(ran_to_end); }
    } ending{att};
    att.begin_replay(n);
    if (!ops || (n && (!mbufs || !frames || !recs)))
        return fail(-EINVAL, "rxg_rx_replay: NULL argument");
    if (!rec_kind_ok(stride)) return fail(-EINVAL, "rxg_rx_replay: stride %u", stride);
    if (n && c->last_n != n)
        return fail(-EINVAL, "rxg_rx_replay: n=%u but the burst to replay (%u of the last launch) had %u frames", n,
                    c->replay_cursor, c->last_n);
    if (n && !c->burst_ok) return fail(-EINVAL, "rxg_rx_replay: the last burst on this context failed");
    // the re-classify launches and the counter correction run on this context's device
    // (a group replays several contexts from one thread, rxg_group.cpp)
    if (int rc = set_device(c)) return rc;
    ReplayLog &log = c->replay;
    log.begin(n, recs, stride);
    // writes the replays of this launch's earlier bursts made, then those since
    if (c->replay_cursor > 0 && !c->launch_writes.empty()) absorb(c, c->launch_writes);
    if (!c->touched.empty()) absorb_touched(c);

    int64_t delta[RXG_NCOUNTERS] = {0};
    std::vector<uint32_t> sel;
    std::vector<rxg_rec16> fix;
    for (uint32_t i = 0; i < n; ++i) {
        if (log.stale(i, frames)) {
            const ReplayLog::Plan p = log.plan(i, frames, n, c->replay_on_device, sel);
            if (p == ReplayLog::kLaunch) {
                if (int rc = reclassify(c, sel, fix)) return rc;
                for (size_t k = 0; k < sel.size(); ++k) refix(c, sel[k], fix[k], delta);
            } else {
                if (c->mir.need_rebuild)  // a reload / growth inside the replay: index first
                    if (int rc = tcb_push(c)) return rc;
                rxg_rec16 r = log.record(i);
                host_classify(c->mir, (const uint8_t *)frames[i], r);
                refix(c, i, r, delta);
            }
            log.done(p, sel.size());
        }
        att.at(i);  // what the handlers take is answered for this packet
        const uint64_t gen_before = c->gen;
        dispatch(c, ops, log.record(i), mbufs[i], (uint8_t *)frames[i]);
        if (c->gen != gen_before) absorb_touched(c);  // the handlers changed the table
    }
    // the launch's next burst is replayed next (a single burst can be replayed again)
    if (c->replay_cursor + 1 < c->last_bursts.size()) select_burst(c, c->replay_cursor + 1);
    bool nz = false;
    for (int k = 0; k < RXG_NCOUNTERS; ++k) nz |= delta[k] != 0;
    if (nz) {  // the corrections, added with the next mirror patch launch (flush_delta)
        for (int k = 0; k < RXG_NCOUNTERS; ++k) c->pend_delta[k] += delta[k];
        c->pend = true;
    }
    ending.ran_to_end = true;
    return 0;
}

extern "C" int rxg_replay_stats(rxg_ctx *c, uint64_t out[4])
{
    if (!c || !out) return fail(-EINVAL, "rxg_replay_stats: NULL argument");
    for (int k = 0; k < 4; ++k) out[k] = c->replay.stats[k];
    return 0;
}
