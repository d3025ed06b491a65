// rxg_replaylog.h — which packets of a burst a table write made stale, and how each is brought
// up to date: the rule of rxg_rx_replay (rxg_replay.cpp).
//
// The burst's records were computed against the table as it stood at the launch.  Every batch of
// tracked writes after that (a WriteSet: those of one handler call, or those made between the
// burst and its replay) gets a number; a record computed at number s is stale when a later write
// touched what it depends on: its tuple (pass 1, old or new tuple of a written slot), or -- for a
// packet pass 1 did not answer -- a LISTENING slot on its dport or the lowest NULL slot (pass 2);
// any write for a frame under 54 bytes; everything after a reload.  Staleness is checked when a
// packet is reached (its header is read there anyway; no per-burst index).  A stale packet is
// re-classified from the host index, or, with everything stale after it, in one launch over a
// selection list (plan()).
//
// Host-only and HIP-free, as rxg_mirror.h and rxg_tablesync.h are: tests/test_replaylog_host.py +
// replaylog_check.cpp play the replay's packet loop over this header on the CPU against the model
// of tests/replay_sel_cases.py, plain and under ASan/UBSan.
#pragma once
#include <stdint.h>

#include <unordered_map>
#include <utility>
#include <vector>

#include "rxg.h"
#include "rxg_common.h"
#include "rxg_mirror.h"

namespace rxg {

// What a batch of table writes can change for the packets of a classified burst.
struct WriteSet {
    std::vector<TupleKey> keys;   // tuples (old and new) of changed slots
    std::vector<int32_t> listen;  // dports whose LISTENING slots changed (pass 2)
    bool all = false;             // whole table replaced
    bool pass2 = false;           // min_null moved (the pass-2 NULL-slot flag)

    bool empty() const { return keys.empty() && listen.empty() && !all && !pass2; }
    void clear()
    {
        keys.clear();
        listen.clear();
        all = pass2 = false;
    }
    void add(const WriteSet &o)
    {
        keys.insert(keys.end(), o.keys.begin(), o.keys.end());
        listen.insert(listen.end(), o.listen.begin(), o.listen.end());
        all |= o.all;
        pass2 |= o.pass2;
    }
};

inline bool rec_is_tcp(const rxg_rec16 &r)
{
    return r.verdict == RXG_V_DISPATCH || r.verdict == RXG_V_RST_NOPCB || r.verdict == RXG_V_RST_LISTEN_NONSYN;
}

// A TCP record that findtcb pass 1 did not answer (listener or no TCB): pass 2 decides it.
inline bool rec_pass2(const rxg_rec16 &r) { return r.tcb_idx < 0 || (r.flags & RXG_F_LISTEN); }

// The replay's written-tuple filter index (16 bits): every packet after a burst's first table
// write is checked against it, so two multiplies rather than the table's seven (tuple_hash;
// 14 -> 6 ns a packet on this container's core); a collision only costs the exact lookup.
inline uint32_t filter_hash(const TupleKey &k) { return (k.ports * 0x9E3779B1u + k.src * 0x85EBCA6Bu + k.dst) >> 16; }

// The pass-1 key of a frame of >= 54 bytes, as the kernel forms it: ports = dport << 16 |
// sport (host order), ipv4_dst as loaded, ipv4_src host order (tcp_tcb.c:134-135,152-155).
inline TupleKey frame_key(const uint8_t *f)
{
    const uint32_t sport = ((uint32_t)f[34] << 8) | f[35], dport = ((uint32_t)f[36] << 8) | f[37];
    const uint32_t dst = (uint32_t)f[30] | ((uint32_t)f[31] << 8) | ((uint32_t)f[32] << 16) | ((uint32_t)f[33] << 24);
    const uint32_t src = ((uint32_t)f[26] << 24) | ((uint32_t)f[27] << 16) | ((uint32_t)f[28] << 8) | f[29];
    return TupleKey{(dport << 16) | sport, dst, src};
}

// A bulk change (a reload, a listener change, min_null moving) that leaves more than this
// many packets of the burst stale re-classifies them in one GPU launch; fewer (and every
// change to single tuples) are answered from the host index as each packet is reached.
inline constexpr uint32_t kHostReclassifyMax = 256;

class ReplayLog {
  public:
    enum Plan { kHost, kLaunch };  // how a stale packet is fixed: from the host index, or sel in one launch
    // marked, host fix-ups, device fix-ups, launches (rxg_replay_stats): over the context's life
    uint64_t stats[4] = {0, 0, 0, 0};

    // A burst of n records as the burst classified them: recs, `stride` bytes apart (RXG_REC8:
    // expanded; else each begins with a rxg_rec16).  No write is known yet.
    void begin(uint32_t n, const void *recs, uint32_t stride)
    {
        cur.resize(n);
        rxg_rec16 *to = cur.data();
        if (stride == RXG_REC8)
            for (uint32_t i = 0; i < n; ++i) rxg_rec8_expand((const rxg_rec8 *)recs + i, to + i);
        else
            for (uint32_t i = 0; i < n; ++i) to[i] = *(const rxg_rec16 *)((const uint8_t *)recs + (size_t)i * stride);
        pkt_seq.assign(n, 0u);  // 0 = as the burst classified it
        wseq = any_seq = all_seq = minnull_seq = bulk_seq = scanned_seq = 0;
        if (!key_seq.empty()) key_seq.clear();
        listen_seq.clear();
        filt_used = false;
    }
    size_t size() const { return cur.size(); }
    const rxg_rec16 &record(size_t j) const { return cur[j]; }
    // packet j still has the record the burst gave it (no re-classification)
    bool as_burst(size_t j) const { return pkt_seq[j] == 0u; }

    // One batch of writes: it gets the next number.
    void absorb(const WriteSet &w)
    {
        ++wseq;
        any_seq = wseq;
        if (w.all) all_seq = bulk_seq = wseq;
        if (w.pass2) minnull_seq = bulk_seq = wseq;
        for (const TupleKey &k : w.keys) {
            key_seq[k] = wseq;
            const uint32_t h = filter_hash(k);
            if (!filt_used) {
                filt.assign(1024, 0ull);
                filt_used = true;
            }
            filt[(h >> 6) & 1023u] |= 1ull << (h & 63u);
        }
        for (int32_t d : w.listen) {
            bool found = false;
            for (auto &e : listen_seq)
                if (e.first == d) {
                    e.second = wseq;
                    found = true;
                }
            if (!found) listen_seq.emplace_back(d, wseq);
            bulk_seq = wseq;
        }
    }

    // Did a write later than packet j's record touch what the record depends on?  The first test
    // is all a burst without table writes pays per packet; frames[j] is read only for a TCP record
    // of a frame of >= 54 bytes.
    bool stale(uint32_t j, void *const *frames) const { return any_seq > pkt_seq[j] && touched_since(j, frames); }

    // Packet i of n is stale.  What is stale from i on is looked for on the device path, for a
    // short frame, or after a bulk change not scanned yet, and goes into one launch (sel, kLaunch)
    // on the device path, for a short frame, or when it is more than kHostReclassifyMax packets;
    // else packet i alone is answered from the host index (kHost).
    Plan plan(uint32_t i, void *const *frames, uint32_t n, bool on_device, std::vector<uint32_t> &sel)
    {
        ++stats[0];
        const bool force = on_device || (cur[i].flags & RXG_F_TRUNC) != 0;
        if (!force && bulk_seq <= scanned_seq) return kHost;
        sel.clear();
        for (uint32_t j = i; j < n; ++j)
            if (stale(j, frames)) sel.push_back(j);
        scanned_seq = wseq;
        return force || sel.size() > kHostReclassifyMax ? kLaunch : kHost;
    }

    // Packet j's record as classified against the table as it stands: fresh up to the current write.
    void fixed(uint32_t j, const rxg_rec16 &r)
    {
        cur[j] = r;
        pkt_seq[j] = wseq;
    }
    // A plan carried out: k packets fixed by its launch, or one on the host.
    void done(Plan p, size_t k)
    {
        if (p == kLaunch) {
            stats[2] += k;
            ++stats[3];
        } else {
            ++stats[1];
        }
    }

  private:
    // stale() for a packet with a write after its record
    bool touched_since(uint32_t j, void *const *frames) const
    {
        const rxg_rec16 &q = cur[j];
        const uint32_t s = pkt_seq[j];
        if (!rec_is_tcp(q)) return false;
        if (all_seq > s || (q.flags & RXG_F_TRUNC)) return true;
        const TupleKey k = frame_key((const uint8_t *)frames[j]);
        if (filt_used) {
            const uint32_t h = filter_hash(k);
            if ((filt[(h >> 6) & 1023u] >> (h & 63u)) & 1ull) {
                auto it = key_seq.find(k);
                if (it != key_seq.end() && it->second > s) return true;
            }
        }
        const int32_t d = (int32_t)(k.ports >> 16);
        if (rec_pass2(q)) {
            if (minnull_seq > s) return true;
            for (const auto &e : listen_seq)
                if (e.first == d && e.second > s) return true;
        }
        return false;
    }

    // the number of the last batch, of the last one at all (= wseq), of the last reload, min_null
    // move and bulk change (a reload, a min_null move, a listener change), and the one plan()'s
    // last scan saw
    uint32_t wseq = 0, any_seq = 0, all_seq = 0, minnull_seq = 0, bulk_seq = 0, scanned_seq = 0;
    std::unordered_map<TupleKey, uint32_t, TupleKeyHash> key_seq;
    std::vector<std::pair<int32_t, uint32_t>> listen_seq;  // (dport, seq): rare
    std::vector<uint64_t> filt;                            // 65 536-bit filter of written tuples
    bool filt_used = false;
    // the working records and the write number each was computed at; kept across bursts
    std::vector<rxg_rec16> cur;
    std::vector<uint32_t> pkt_seq;
};

}  // namespace rxg
