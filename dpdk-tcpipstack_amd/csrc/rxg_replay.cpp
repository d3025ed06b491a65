// rxg_replay.cpp — the per-packet replay of a classified burst into the caller's handlers
// (rxg_rx_replay: the reference's ether_in -> ip_in -> tcp_in order, re-classifying what a
// handler's table write changed), the payload hand-off (rxg_payload_gather_dev, rxg_rcv_set,
// rxg_payload_take), the prebuilt resets' hand-out (rxg_reset_attach, rxg_reset_take), the
// parsed options' (rxg_rx_opts_attach, rxg_rx_opt_current), the prebuilt ACKs' (rxg_acks_attach,
// rxg_ack_take) and the one-frame rxg_ether_in.
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
    if (c->pm_ev) HIP_OK(hipStreamWaitEvent(st, c->pm_ev, 0));
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
    // rxg_payload_take fetches the descriptors on its first call after this gather
    if (!c->pm_ev) HIP_OK(hipEventCreateWithFlags(&c->pm_ev, hipEventDisableTiming));
    HIP_OK(hipEventRecord(c->pm_ev, st));
    c->d_pm = o->msgs;
    c->pm_used = o->arena_used;
    c->pm_n = n;
    c->pm_pending = true;
    c->pm_poisoned = false;
    return 0;
}

extern "C" int rxg_rcv_set(rxg_ctx *c, int32_t idx, uint32_t cur_seq, uint32_t pairs_pending)
{
    if (!c) return fail(-EINVAL, "rxg_rcv_set: ctx NULL");
    if (idx < 0 || idx >= kMaxTcbs) return fail(-EINVAL, "rxg_rcv_set: index %d", idx);
    if ((size_t)idx >= c->rcv_state.size()) {
        c->rcv_state.resize((size_t)idx + 1, 0);
        c->rcv_cur.resize((size_t)idx + 1, 0);
    }
    c->rcv_cur[idx] = cur_seq;
    c->rcv_state[idx] = pairs_pending ? 2 : 1;
    return 0;
}

// PushData (tcp_windows.c:341-358) with an empty SeqPairs list and
// CurrentSequenceNumber == seq: the out-of-window test needs SeqPairs (:345) and is
// skipped; the duplicate test (:349) drops iff cur > seq + Length (u32); AdjustPair puts
// the one pair at the head (:42-110, returns seq + Length + FIN); GetData pops it with
// offset 0 and copies Length bytes (:158-180) -> one message of exactly this payload.
extern "C" int rxg_payload_take(rxg_ctx *c, int32_t idx, uint32_t seq, uint32_t length, rxg_payload_msg *msg)
{
    if (!c) return fail(-EINVAL, "rxg_payload_take: ctx NULL");
    const int64_t pos = c->attached.pos;
    if (pos < 0 || (uint64_t)pos >= c->pm_n || length == 0 || length > 0xFFFFu) return 0;
    if (c->pm_pending) {  // first take after the gather: fetch the burst's descriptors
        if (int rc = set_device(c)) return rc;
        HIP_OK(hipEventSynchronize(c->pm_ev));
        if (c->pm_n > c->h_pm_cap) {
            if (c->h_pm) HIP_OK(hipHostFree(c->h_pm));
            c->h_pm = nullptr;
            c->h_pm_cap = 0;
            HIP_OK(hipHostMalloc((void **)&c->h_pm, (size_t)c->pm_n * sizeof(rxg_payload_msg), hipHostMallocDefault));
            c->h_pm_cap = c->pm_n;
        }
        uint64_t used = 0;
        HIP_OK(hipMemcpyAsync(c->h_pm, c->d_pm, (size_t)c->pm_n * sizeof(rxg_payload_msg), hipMemcpyDeviceToHost,
                              c->stream));
        if (c->pm_used)  // (a fused burst, rxg_rx_burst_payload_dev, has no look-back to time out)
            HIP_OK(hipMemcpyAsync(&used, c->pm_used, sizeof used, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        c->pm_pending = false;
        // a gather whose look-back timed out (arena_used = ~0) placed payloads at unknown
        // offsets: nothing of that burst is handed out (the stack's own PushData runs)
        c->pm_poisoned = used == ~0ull;
    }
    if (c->pm_poisoned) return 0;
    const rxg_payload_msg &m = c->h_pm[pos];
    if (!(m.flags & RXG_PM_GATHERED) || m.len != length) return 0;
    if (idx < 0 || (size_t)idx >= c->rcv_state.size() || c->rcv_state[idx] != 1 || c->rcv_cur[idx] != seq)
        return 0;
    if (seq > (uint32_t)(seq + length)) return 0;  // the duplicate test drops it
    if (seq == 0) return 0;  // GetData asserts CurrentSequenceNumber != 0 (:151): the stack's own code
    c->rcv_cur[idx] = seq + length;
    if (msg) *msg = m;
    return 1;
}

// ------------------------------------------------------------------ prebuilt resets ---
extern "C" int rxg_reset_attach(rxg_ctx *c, void *resets_host, const uint32_t *idx_host, uint64_t nbuilt)
{
    if (!c || (nbuilt && (!resets_host || !idx_host)))
        return fail(-EINVAL, "rxg_reset_attach: NULL argument");
    ReplayAttached &a = c->attached;
    a.rst_host = nbuilt ? (uint8_t *)resets_host : nullptr;
    a.rst_idx = nbuilt ? idx_host : nullptr;
    a.rst_n = nbuilt;
    a.rst_cur = 0;
    return 0;
}

// idx_host ascends (resets come out in packet order) and the replay's position only grows:
// one cursor, moved to the first entry at or after the packet being replayed.  An entry
// passed over belongs to a frame that no longer wants its reset (re-classified to DISPATCH,
// or dropped by the checksum verify).
extern "C" int rxg_reset_take(rxg_ctx *c, uint16_t ip_id, void **frame_out)
{
    if (!c || !frame_out) return fail(-EINVAL, "rxg_reset_take: NULL argument");
    ReplayAttached &a = c->attached;
    const int64_t pos = a.pos;
    if (pos < 0 || !a.rst_host) return 0;
    while (a.rst_cur < a.rst_n && (int64_t)a.rst_idx[a.rst_cur] < pos) ++a.rst_cur;
    if (a.rst_cur >= a.rst_n || (int64_t)a.rst_idx[a.rst_cur] != pos) return 0;
    uint8_t *f = a.rst_host + 64u * a.rst_cur;
    if ((uint16_t)(f[18] | (f[19] << 8)) != ip_id) rxg_reset_set_id(f, ip_id);
    *frame_out = f;
    return 1;
}

// ------------------------------------------------------------------ parsed options ---
extern "C" int rxg_rx_opts_attach(rxg_ctx *c, const rxg_rx_opt *opts_host, uint32_t n)
{
    if (!c || (n && !opts_host)) return fail(-EINVAL, "rxg_rx_opts_attach: NULL argument");
    c->attached.opt_host = n ? opts_host : nullptr;
    c->attached.opt_n = n;
    return 0;
}

// The record of the attached copy for the packet being replayed: options do not depend on the
// mirror, so the record of a packet the replay re-classified is as good as any other's.
extern "C" int rxg_rx_opt_current(rxg_ctx *c, const rxg_rx_opt **out)
{
    if (!c || !out) return fail(-EINVAL, "rxg_rx_opt_current: NULL argument");
    const ReplayAttached &a = c->attached;
    const int64_t pos = a.pos;
    if (pos < 0 || !a.opt_host || !a.opt_live || pos >= (int64_t)a.opt_n) return 0;
    *out = a.opt_host + pos;
    return 1;
}

// ---------------------------------------------------------------- flow summaries ---
extern "C" int rxg_flow_sums_attach(rxg_ctx *c, const rxg_flow_sum *sums_host, uint64_t m)
{
    if (!c || (m && !sums_host)) return fail(-EINVAL, "rxg_flow_sums_attach: NULL argument");
    for (uint64_t k = 1; k < m; ++k)
        if (sums_host[k].tcb_idx <= sums_host[k - 1].tcb_idx)
            return fail(-EINVAL, "rxg_flow_sums_attach: entry %llu is not above its predecessor's tcb_idx",
                        (unsigned long long)k);
    c->attached.fs_host = m ? sums_host : nullptr;
    c->attached.fs_m = m;
    return 0;
}

// The packet being replayed, if its record is still the burst's (ReplayLog::as_burst: not
// re-classified) and a DISPATCH to a flow of the attached list that covers its index.
extern "C" int rxg_flow_sum_current(rxg_ctx *c, const rxg_flow_sum **out, uint32_t *pkt_idx)
{
    if (!c || !out || !pkt_idx) return fail(-EINVAL, "rxg_flow_sum_current: NULL argument");
    const ReplayAttached &a = c->attached;
    const int64_t pos = a.pos;
    if (pos < 0 || !a.fs_host || (uint64_t)pos >= c->replay.size()) return 0;
    const rxg_rec16 &r = c->replay.record((size_t)pos);
    if (!c->replay.as_burst((size_t)pos) || r.verdict != RXG_V_DISPATCH) return 0;
    const rxg_flow_sum *lo = a.fs_host, *hi = a.fs_host + a.fs_m;
    const rxg_flow_sum *s =
        std::lower_bound(lo, hi, r.tcb_idx, [](const rxg_flow_sum &e, int32_t t) { return e.tcb_idx < t; });
    if (s == hi || s->tcb_idx != r.tcb_idx || (uint64_t)pos < s->first_idx || (uint64_t)pos > s->last_idx) return 0;
    *out = s;
    *pkt_idx = (uint32_t)pos;
    return 1;
}

// ------------------------------------------------------------------- flow trains ---
extern "C" int rxg_flow_trains_attach(rxg_ctx *c, const uint32_t *order_host, uint64_t nseg,
                                      const rxg_flow_train *trains_host, uint64_t ntrains)
{
    if (!c || (nseg && !order_host) || (ntrains && !trains_host))
        return fail(-EINVAL, "rxg_flow_trains_attach: NULL argument");
    uint64_t at = 0;
    for (uint64_t k = 0; k < ntrains; ++k) {
        const rxg_flow_train &t = trains_host[k];
        if (t.first != at || t.nseg == 0 || (k && t.tcb_idx < trains_host[k - 1].tcb_idx))
            return fail(-EINVAL, "rxg_flow_trains_attach: train %llu does not start where its predecessor ended "
                                 "(first %u, nseg %u, expected first %llu)",
                        (unsigned long long)k, t.first, t.nseg, (unsigned long long)at);
        at += t.nseg;
    }
    ReplayAttached &a = c->attached;
    a.ft_order = nseg ? order_host : nullptr;
    a.ft_trains = ntrains ? trains_host : nullptr;
    a.ft_nseg = nseg;
    a.ft_ntrains = ntrains;
    return 0;
}

// The packet being replayed, if its record is still the burst's (ReplayLog::as_burst: not
// re-classified) and a DISPATCH: the attached trains of its flow are found by tcb_idx, the packet
// among the flow's segments (ascending packet indices), and its train by that position.
extern "C" int rxg_flow_train_current(rxg_ctx *c, const rxg_flow_train **out, uint32_t *pos_out)
{
    if (!c || !out || !pos_out) return fail(-EINVAL, "rxg_flow_train_current: NULL argument");
    const ReplayAttached &a = c->attached;
    const int64_t pos = a.pos;
    if (pos < 0 || !a.ft_order || !a.ft_trains || (uint64_t)pos >= c->replay.size()) return 0;
    const rxg_rec16 &r = c->replay.record((size_t)pos);
    if (!c->replay.as_burst((size_t)pos) || r.verdict != RXG_V_DISPATCH) return 0;
    const rxg_flow_train *lo = a.ft_trains, *hi = a.ft_trains + a.ft_ntrains;
    const rxg_flow_train *tl =
        std::lower_bound(lo, hi, r.tcb_idx, [](const rxg_flow_train &e, int32_t t) { return e.tcb_idx < t; });
    const rxg_flow_train *th =
        std::upper_bound(tl, hi, r.tcb_idx, [](int32_t t, const rxg_flow_train &e) { return t < e.tcb_idx; });
    if (tl == th) return 0;
    const uint64_t s0 = tl->first, s1 = std::min<uint64_t>((uint64_t)(th - 1)->first + (th - 1)->nseg, a.ft_nseg);
    if (s0 >= s1) return 0;
    const uint32_t *seg = std::lower_bound(a.ft_order + s0, a.ft_order + s1, (uint32_t)pos);
    if (seg == a.ft_order + s1 || *seg != (uint32_t)pos) return 0;
    const uint64_t q = (uint64_t)(seg - a.ft_order);
    // the last train of the flow that starts at or before q
    const rxg_flow_train *t =
        std::upper_bound(tl, th, q, [](uint64_t v, const rxg_flow_train &e) { return v < e.first; }) - 1;
    if ((uint64_t)t->first + t->nseg > a.ft_nseg) return 0;  // order was capped inside this train
    *out = t;
    *pos_out = (uint32_t)(q - t->first);
    return 1;
}

// ------------------------------------------------------------------ prebuilt ACKs ---
extern "C" int rxg_acks_attach(rxg_ctx *c, const rxg_ack *acks_host, void *frames_host, uint32_t stride, uint64_t nacks)
{
    if (!c || (nacks && (!acks_host || !frames_host || !stride)))
        return fail(-EINVAL, "rxg_acks_attach: NULL argument or stride 0");
    for (uint64_t a = 1; a < nacks; ++a)
        if (acks_host[a].tcb_idx <= acks_host[a - 1].tcb_idx)
            return fail(-EINVAL, "rxg_acks_attach: entry %llu is not above its predecessor's tcb_idx",
                        (unsigned long long)a);
    ReplayAttached &a = c->attached;
    a.acks_detach();
    if (!nacks) return 0;
    a.ak_acks = acks_host;
    a.ak_frames = (uint8_t *)frames_host;
    a.ak_stride = stride;
    a.ak_n = nacks;
    a.ak_phase = 1;
    return 0;
}

// The attached ACK of tcb_idx, if it still says what the stack's state says and nothing voids
// it: no packet re-classified to or from the TCB, no write to its slot (the slot's tuple is among
// the written ones, or the slot is gone), no whole-table change -- in the replay, or since it
// returned (the writes not yet absorbed: rxg_ctx::touched, kept until the next burst).
extern "C" int rxg_ack_take(rxg_ctx *c, int32_t tcb_idx, uint32_t snd_nxt, uint32_t rcv_ack, void **frame_out)
{
    if (!c || !frame_out) return fail(-EINVAL, "rxg_ack_take: NULL argument");
    const ReplayAttached &a = c->attached;
    if (a.ak_phase != 2u || a.ak_void_all) return 0;
    const rxg_ack *lo = a.ak_acks, *hi = a.ak_acks + a.ak_n;
    const rxg_ack *e = std::lower_bound(lo, hi, tcb_idx, [](const rxg_ack &x, int32_t t) { return x.tcb_idx < t; });
    if (e == hi || e->tcb_idx != tcb_idx || e->seq != snd_nxt || e->ack != rcv_ack) return 0;
    if (tcb_idx < 0 || tcb_idx >= c->mir.ntcb() || !c->mir.live[tcb_idx]) return 0;
    TupleKey k;
    if (!tcb_key(c->mir.tcb[tcb_idx], k)) return 0;
    if (a.ak_void_tcb.count(tcb_idx) || a.ak_void_keys.count(k)) return 0;
    if (c->touched.all || std::find(c->touched.keys.begin(), c->touched.keys.end(), k) != c->touched.keys.end()) return 0;
    *frame_out = a.ak_frames + (size_t)(e - lo) * a.ak_stride;
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

// One batch of table writes into the replay's log; with prebuilt ACKs handed out (ak_on), what
// of it voids one (rxg_ack_take).
static void absorb(rxg_ctx *c, bool ak_on, const WriteSet &w)
{
    if (ak_on) {
        c->attached.ak_void_all |= w.all;
        c->attached.ak_void_keys.insert(w.keys.begin(), w.keys.end());
    }
    c->replay.absorb(w);
}

// The tracked writes since the last absorb; logged for the launch's later bursts, whose records
// were computed before them too.
static void absorb_touched(rxg_ctx *c, bool ak_on)
{
    c->launch_writes.add(c->touched);
    absorb(c, ak_on, c->touched);
    c->touched.clear();
}

// Packet j's record becomes r: the counter corrections, the TCBs whose prebuilt ACK that voids.
static void refix(rxg_ctx *c, bool ak_on, uint32_t j, const rxg_rec16 &r, int64_t *delta)
{
    const rxg_rec16 &old = c->replay.record(j);
    tcp_record_counters(old, -1, delta);
    tcp_record_counters(r, +1, delta);
    if (ak_on) {
        c->attached.ak_void_tcb.insert(old.tcb_idx);
        c->attached.ak_void_tcb.insert(r.tcb_idx);
    }
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
    // on every way out: no packet is being replayed, and what was attached for this replay is no
    // longer named
    struct PosGuard {
        ReplayAttached &a;
        bool done = false;  // the replay ran to its end
        ~PosGuard()
        {
            // prebuilt ACKs (rxg_acks_attach) are only handed out after a replay that saw the whole
            // burst: one that fails, in its argument checks or later, ends the attachment
            if (!done) a.acks_detach();
            a.end_of_replay();
        }
    } pos_guard{att};
    // the prebuilt ACKs (rxg_acks_attach) outlive one replay: an attachment that has had its
    // replay ends here, a fresh one belongs to this burst (and ends with it if it fails: pos_guard)
    if (att.ak_phase == 2u) att.acks_detach();
    else if (att.ak_phase == 1u) att.ak_phase = 2u;
    const bool ak_on = att.ak_phase == 2u;
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
    att.opt_live = att.opt_host && att.opt_n == n;  // (rxg_rx_opts_attach) the copy is this burst's
    ReplayLog &log = c->replay;
    log.begin(n, recs, stride);
    // writes the replays of this launch's earlier bursts made, then those since
    if (c->replay_cursor > 0 && !c->launch_writes.empty()) absorb(c, ak_on, c->launch_writes);
    if (!c->touched.empty()) absorb_touched(c, ak_on);

    int64_t delta[RXG_NCOUNTERS] = {0};
    std::vector<uint32_t> sel;
    std::vector<rxg_rec16> fix;
    for (uint32_t i = 0; i < n; ++i) {
        if (log.stale(i, frames)) {
            const ReplayLog::Plan p = log.plan(i, frames, n, c->replay_on_device, sel);
            if (p == ReplayLog::kLaunch) {
                if (int rc = reclassify(c, sel, fix)) return rc;
                for (size_t k = 0; k < sel.size(); ++k) refix(c, ak_on, sel[k], fix[k], delta);
            } else {
                if (c->mir.need_rebuild)  // a reload / growth inside the replay: index first
                    if (int rc = tcb_push(c)) return rc;
                rxg_rec16 r = log.record(i);
                host_classify(c->mir, (const uint8_t *)frames[i], r);
                refix(c, ak_on, i, r, delta);
            }
            log.done(p, sel.size());
        }
        att.pos = i;  // rxg_payload_take answers for this packet
        const uint64_t gen_before = c->gen;
        dispatch(c, ops, log.record(i), mbufs[i], (uint8_t *)frames[i]);
        if (c->gen != gen_before) absorb_touched(c, ak_on);  // the handlers changed the table
    }
    // the launch's next burst is replayed next (a single burst can be replayed again)
    if (c->replay_cursor + 1 < c->last_bursts.size()) select_burst(c, c->replay_cursor + 1);
    bool nz = false;
    for (int k = 0; k < RXG_NCOUNTERS; ++k) nz |= delta[k] != 0;
    if (nz) {  // the corrections, added with the next mirror patch launch (flush_delta)
        for (int k = 0; k < RXG_NCOUNTERS; ++k) c->pend_delta[k] += delta[k];
        c->pend = true;
    }
    pos_guard.done = true;
    return 0;
}

extern "C" int rxg_replay_stats(rxg_ctx *c, uint64_t out[4])
{
    if (!c || !out) return fail(-EINVAL, "rxg_replay_stats: NULL argument");
    for (int k = 0; k < 4; ++k) out[k] = c->replay.stats[k];
    return 0;
}
