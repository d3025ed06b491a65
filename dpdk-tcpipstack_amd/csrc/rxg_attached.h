// rxg_attached.h — what a replay hands out to the handlers it calls: the host copies a caller
// attached for the replay that follows (prebuilt resets, parsed options, flow summaries, flow
// trains, prebuilt ACKs), answered for the packet rxg_rx_replay is running, and the receive-window
// mirror rxg_payload_take answers from.  The rules behind rxg_reset_take, rxg_rx_opt_current,
// rxg_flow_sum_current, rxg_flow_train_current, rxg_ack_take, rxg_rcv_set and rxg_payload_take
// (include/rxg.h; the C functions in rxg_replay.cpp check their arguments, word the error and make
// one call here).
//
// Host-only and HIP-free, as rxg_replaylog.h is: tests/test_attached_host.py + attached_check.cpp
// drive these types on the CPU against the model of tests/attached_cases.py, plain and under
// ASan/UBSan, every attached array a heap block of its own length.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <unordered_set>
#include <vector>

#include "rxg.h"
#include "rxg_mirror.h"
#include "rxg_replaylog.h"

namespace rxg {

// The receive-window mirror (rxg_rcv_set): per TCB, ReceiveWindow.CurrentSequenceNumber and
// whether the window is known and its SeqPairs list empty.
class RcvWindow {
  public:
    // the table grows to hold idx (a negative one names no TCB: nothing is set)
    void set(int32_t idx, uint32_t cur_seq, bool pairs_pending)
    {
        if (idx < 0) return;
        if ((size_t)idx >= state.size()) {
            state.resize((size_t)idx + 1, kUnknown);
            cur.resize((size_t)idx + 1, 0);
        }
        cur[idx] = cur_seq;
        state[idx] = pairs_pending ? kPairs : kNoPairs;
    }
    void forget(int32_t idx)  // FreeWindow (rxg_tcb_remove)
    {
        if (idx >= 0 && (size_t)idx < state.size()) state[idx] = kUnknown;
    }
    void clear()  // rxg_tcb_load
    {
        cur.clear();
        state.clear();
    }
    size_t size() const { return state.size(); }

    // PushData (tcp_windows.c:341-358) with an empty SeqPairs list and CurrentSequenceNumber ==
    // seq, for the segment the gather described as m: the out-of-window test needs SeqPairs (:345)
    // and is skipped; the duplicate test (:349) drops iff cur > seq + Length (u32); AdjustPair puts
    // the one pair at the head (:42-110, returns seq + Length + FIN); GetData pops it with offset 0
    // and copies Length bytes (:158-180) -> one message of exactly this payload.  true: the window
    // advances to seq + length and m is the message.
    bool take(int32_t idx, uint32_t seq, uint32_t length, const rxg_payload_msg &m)
    {
        if (!(m.flags & RXG_PM_GATHERED) || m.len != length) return false;
        if (idx < 0 || (size_t)idx >= state.size() || state[idx] != kNoPairs || cur[idx] != seq) return false;
        if (seq > (uint32_t)(seq + length)) return false;  // the duplicate test drops it
        if (seq == 0) return false;  // GetData asserts CurrentSequenceNumber != 0 (:151): the stack's own code
        cur[idx] = seq + length;
        return true;
    }

  private:
    enum : uint8_t { kUnknown, kNoPairs, kPairs };
    std::vector<uint32_t> cur;
    std::vector<uint8_t> state;
};

class ReplayAttached {
  public:
    // ------------------------------------------------------------- the replay's life cycle ---
    // rxg_rx_replay of a burst of n packets begins.  The prebuilt ACKs outlive one replay: an
    // attachment that has had its replay ends here, a fresh one belongs to this burst.
    void begin_replay(uint32_t n)
    {
        if (ak_phase == kHandedOut) acks_detach();
        else if (ak_phase == kWaiting) ak_phase = kHandedOut;
        opt_live = opt_host && opt_n == n;  // the attached options are this burst's
    }
    // the packet whose handlers run next
    void at(uint32_t i) { pos = i; }
    // -1: no packet is being replayed
    int64_t position() const { return pos; }
    // A batch of table writes the replay absorbed: with ACKs handed out, what of it voids one.
    // (This test and refixed's are all a replay without attached ACKs pays: the sets stay out of line.)
    void wrote(const WriteSet &w)
    {
        if (ak_phase == kHandedOut) void_written(w);
    }
    // A packet's record re-classified from old_rec to new_rec: neither TCB's ACK is handed out.
    void refixed(const rxg_rec16 &old_rec, const rxg_rec16 &new_rec)
    {
        if (ak_phase == kHandedOut) void_tcbs(old_rec.tcb_idx, new_rec.tcb_idx);
    }
    // The replay returns: no packet is being replayed, and what was attached for it is no longer
    // named.  The ACKs stay, unless the replay did not see the whole burst (it failed, in its
    // argument checks or later).
    void end_replay(bool ran_to_end)
    {
        if (!ran_to_end) acks_detach();
        pos = -1;
        rst_host = nullptr;
        rst_idx = nullptr;
        rst_n = rst_cur = 0;
        opt_host = nullptr;
        opt_n = 0;
        opt_live = false;
        fs_host = nullptr;
        fs_m = 0;
        ft_order = nullptr;
        ft_trains = nullptr;
        ft_nseg = ft_ntrains = 0;
    }

    // ------------------------------------------------------------------ prebuilt resets ---
    // n 64-byte resets and the packet index of each, ascending (rxg_reset_attach)
    void attach_resets(void *host, const uint32_t *idx, uint64_t n)
    {
        rst_host = n ? (uint8_t *)host : nullptr;
        rst_idx = n ? idx : nullptr;
        rst_n = n;
        rst_cur = 0;
    }
    // The reset prebuilt for the packet being replayed, carrying ip_id; NULL if there is none.
    // The indices ascend and the replay's position only grows: one cursor, moved to the first entry
    // at or after the packet.  An entry passed over belongs to a frame that no longer wants its
    // reset (re-classified to DISPATCH, or dropped by the checksum verify).
    uint8_t *take_reset(uint16_t ip_id)
    {
        if (pos < 0 || !rst_host) return nullptr;
        while (rst_cur < rst_n && (int64_t)rst_idx[rst_cur] < pos) ++rst_cur;
        if (rst_cur >= rst_n || (int64_t)rst_idx[rst_cur] != pos) return nullptr;
        uint8_t *f = rst_host + 64u * rst_cur;
        if ((uint16_t)(f[18] | (f[19] << 8)) != ip_id) rxg_reset_set_id(f, ip_id);
        return f;
    }

    // ------------------------------------------------------------------- parsed options ---
    // a rxg_rx_opts_dev call's n records (rxg_rx_opts_attach)
    void attach_opts(const rxg_rx_opt *host, uint32_t n)
    {
        opt_host = n ? host : nullptr;
        opt_n = n;
    }
    // The record of the packet being replayed, if the replayed burst has as many frames as were
    // attached; NULL otherwise.  Options do not depend on the mirror, so the record of a packet the
    // replay re-classified is as good as any other's.
    const rxg_rx_opt *opt_current() const
    {
        if (pos < 0 || !opt_host || !opt_live || pos >= (int64_t)opt_n) return nullptr;
        return opt_host + pos;
    }

    // ------------------------------------------------------------------- flow summaries ---
    // m summaries, tcb_idx strictly ascending (rxg_flow_sums_attach).  false, nothing changed:
    // entry *bad_k is not above its predecessor's.
    bool attach_flow_sums(const rxg_flow_sum *host, uint64_t m, uint64_t *bad_k)
    {
        for (uint64_t k = 1; k < m; ++k)
            if (host[k].tcb_idx <= host[k - 1].tcb_idx) {
                *bad_k = k;
                return false;
            }
        fs_host = m ? host : nullptr;
        fs_m = m;
        return true;
    }
    // The summary of the flow of the packet being replayed and, in *pkt, the packet's index: if its
    // record is still the burst's (not re-classified) and a DISPATCH to a flow of the attached list
    // that covers its index.  NULL otherwise.
    const rxg_flow_sum *flow_sum_current(const ReplayLog &log, uint32_t *pkt) const
    {
        if (pos < 0 || !fs_host) return nullptr;
        const rxg_rec16 *r = burst_dispatch(log);
        if (!r) return nullptr;
        const int32_t tcb = r->tcb_idx;
        const rxg_flow_sum *hi = fs_host + fs_m;
        const rxg_flow_sum *s =
            std::lower_bound(fs_host, hi, tcb, [](const rxg_flow_sum &e, int32_t t) { return e.tcb_idx < t; });
        if (s == hi || s->tcb_idx != tcb || (uint64_t)pos < s->first_idx || (uint64_t)pos > s->last_idx) return nullptr;
        *pkt = (uint32_t)pos;
        return s;
    }

    // ---------------------------------------------------------------------- flow trains ---
    // nseg packet indices grouped by flow and ntrains trains that tile them in order
    // (rxg_flow_trains_attach): train k starts where train k - 1 ended, train 0 at 0, nseg >= 1
    // each, tcb_idx never descending; trains past nseg may follow.  false, nothing changed: train
    // *bad_k does not start at *expected_first, is empty, or descends.
    bool attach_flow_trains(const uint32_t *order, uint64_t nseg, const rxg_flow_train *trains, uint64_t ntrains,
                            uint64_t *bad_k, uint64_t *expected_first)
    {
        uint64_t first = 0;
        for (uint64_t k = 0; k < ntrains; ++k) {
            const rxg_flow_train &t = trains[k];
            if (t.first != first || t.nseg == 0 || (k && t.tcb_idx < trains[k - 1].tcb_idx)) {
                *bad_k = k;
                *expected_first = first;
                return false;
            }
            first += t.nseg;
        }
        ft_order = nseg ? order : nullptr;
        ft_trains = ntrains ? trains : nullptr;
        ft_nseg = nseg;
        ft_ntrains = ntrains;
        return true;
    }
    // The train of the packet being replayed and, in *pos_in_train, its place in it: if its record
    // is still the burst's (not re-classified) and a DISPATCH.  The attached trains of its flow are
    // found by tcb_idx, the packet among the flow's segments (ascending packet indices), and its
    // train by that position.  NULL otherwise, also for a train that order was capped inside.
    const rxg_flow_train *flow_train_current(const ReplayLog &log, uint32_t *pos_in_train) const
    {
        if (pos < 0 || !ft_order || !ft_trains) return nullptr;
        const rxg_rec16 *r = burst_dispatch(log);
        if (!r) return nullptr;
        const int32_t tcb = r->tcb_idx;
        const rxg_flow_train *hi = ft_trains + ft_ntrains;
        const rxg_flow_train *tl =
            std::lower_bound(ft_trains, hi, tcb, [](const rxg_flow_train &e, int32_t t) { return e.tcb_idx < t; });
        const rxg_flow_train *th =
            std::upper_bound(tl, hi, tcb, [](int32_t t, const rxg_flow_train &e) { return t < e.tcb_idx; });
        if (tl == th) return nullptr;
        const uint64_t s0 = tl->first, s1 = std::min<uint64_t>((uint64_t)(th - 1)->first + (th - 1)->nseg, ft_nseg);
        if (s0 >= s1) return nullptr;
        const uint32_t *seg = std::lower_bound(ft_order + s0, ft_order + s1, (uint32_t)pos);
        if (seg == ft_order + s1 || *seg != (uint32_t)pos) return nullptr;
        const uint64_t q = (uint64_t)(seg - ft_order);
        // the last train of the flow that starts at or before q
        const rxg_flow_train *t =
            std::upper_bound(tl, th, q, [](uint64_t v, const rxg_flow_train &e) { return v < e.first; }) - 1;
        if ((uint64_t)t->first + t->nseg > ft_nseg) return nullptr;  // order was capped inside this train
        *pos_in_train = (uint32_t)(q - t->first);
        return t;
    }

    // -------------------------------------------------------------------- prebuilt ACKs ---
    // n ACKs, tcb_idx strictly ascending, ACK a's frame at frames + a * stride (rxg_acks_attach):
    // replaces the attachment there was, and waits for its replay.  false, nothing changed: entry
    // *bad_k is not above its predecessor's.
    bool attach_acks(const rxg_ack *acks, void *frames, uint32_t stride, uint64_t n, uint64_t *bad_k)
    {
        for (uint64_t a = 1; a < n; ++a)
            if (acks[a].tcb_idx <= acks[a - 1].tcb_idx) {
                *bad_k = a;
                return false;
            }
        acks_detach();
        if (!n) return true;
        ak_acks = acks;
        ak_frames = (uint8_t *)frames;
        ak_stride = stride;
        ak_n = n;
        ak_phase = kWaiting;
        return true;
    }
    // The attached ACK frame of tcb_idx, once its replay has begun (and after it returned), if it
    // still says what the stack's state says (snd_nxt, rcv_ack) and nothing voids it: no packet
    // re-classified to or from the TCB, no write to its slot (the slot's tuple is among the written
    // ones, or the slot is gone), no whole-table change -- in the replay (wrote, refixed), or since
    // it returned (touched: the writes no replay has absorbed yet).  NULL otherwise.
    uint8_t *ack_take(int32_t tcb_idx, uint32_t snd_nxt, uint32_t rcv_ack, const TcbMirror &mir,
                      const WriteSet &touched) const
    {
        if (ak_phase != kHandedOut || ak_void_all) return nullptr;
        const rxg_ack *hi = ak_acks + ak_n;
        const rxg_ack *e =
            std::lower_bound(ak_acks, hi, tcb_idx, [](const rxg_ack &x, int32_t t) { return x.tcb_idx < t; });
        if (e == hi || e->tcb_idx != tcb_idx || e->seq != snd_nxt || e->ack != rcv_ack) return nullptr;
        if (tcb_idx < 0 || tcb_idx >= mir.ntcb() || !mir.live[tcb_idx]) return nullptr;
        TupleKey k;
        if (!tcb_key(mir.tcb[tcb_idx], k)) return nullptr;
        if (ak_void_tcb.count(tcb_idx) || ak_void_keys.count(k)) return nullptr;
        if (touched.all || std::find(touched.keys.begin(), touched.keys.end(), k) != touched.keys.end()) return nullptr;
        return ak_frames + (size_t)(e - ak_acks) * ak_stride;
    }

  private:
    // the record of the packet being replayed (pos >= 0) if it is the burst's own and a DISPATCH
    const rxg_rec16 *burst_dispatch(const ReplayLog &log) const
    {
        if ((uint64_t)pos >= log.size() || !log.as_burst((size_t)pos)) return nullptr;
        const rxg_rec16 &r = log.record((size_t)pos);
        return r.verdict == RXG_V_DISPATCH ? &r : nullptr;
    }
    __attribute__((noinline)) void void_written(const WriteSet &w)
    {
        ak_void_all |= w.all;
        ak_void_keys.insert(w.keys.begin(), w.keys.end());
    }
    __attribute__((noinline)) void void_tcbs(int32_t from, int32_t to)
    {
        ak_void_tcb.insert(from);
        ak_void_tcb.insert(to);
    }
    void acks_detach()
    {
        ak_acks = nullptr;
        ak_frames = nullptr;
        ak_n = 0;
        ak_stride = 0;
        ak_phase = kNone;
        ak_void_tcb.clear();
        ak_void_keys.clear();
        ak_void_all = false;
    }

    int64_t pos = -1;  // packet whose handlers rxg_rx_replay is running
    uint8_t *rst_host = nullptr;
    const uint32_t *rst_idx = nullptr;
    uint64_t rst_n = 0, rst_cur = 0;  // rst_cur: take_reset's cursor
    const rxg_rx_opt *opt_host = nullptr;
    uint32_t opt_n = 0;
    bool opt_live = false;  // the running replay's burst has opt_n frames
    const rxg_flow_sum *fs_host = nullptr;
    uint64_t fs_m = 0;
    const uint32_t *ft_order = nullptr;
    const rxg_flow_train *ft_trains = nullptr;
    uint64_t ft_nseg = 0, ft_ntrains = 0;
    // The ACKs' attachment: waiting for its replay; handed out from that replay's begin on, also
    // after it returned, until the next replay, attach or failure ends it.  What the replay saw
    // that voids a prebuilt ACK: the TCBs a re-classification took a packet from or gave one to,
    // the tuples of written slots, a whole-table change.
    enum AckPhase : uint8_t { kNone, kWaiting, kHandedOut };
    const rxg_ack *ak_acks = nullptr;
    uint8_t *ak_frames = nullptr;
    uint64_t ak_n = 0;
    uint32_t ak_stride = 0;
    AckPhase ak_phase = kNone;
    std::unordered_set<int32_t> ak_void_tcb;
    std::unordered_set<TupleKey, TupleKeyHash> ak_void_keys;
    bool ak_void_all = false;
};

}  // namespace rxg
