// rxg_flowtrain.cpp — rxg_flow_trains_host: the flow-train rule of rxg.h applied to a burst in
// host memory (rxg_rx_burst's records and the caller's frames), without a context or a GPU.
// The device form is rxg_flowtrain.hip.
#include <cerrno>
#include <cstddef>
#include <algorithm>
#include <new>
#include <vector>

#include "rxg.h"

static_assert(sizeof(rxg_flow_train) == 32 && offsetof(rxg_flow_train, bytes) == 16 &&
                  offsetof(rxg_flow_train, next_ack) == 24,
              "rxg_flow_train layout");

namespace {

struct Seg {
    int32_t tcb;
    uint32_t idx, seq, datalen;
    bool fin;
    bool wraps() const { return (uint64_t)seq + datalen >= (1ull << 32); }
};

// big-endian frame[at .. at + 4), bytes at or beyond len read as zero
inline uint32_t be32_cut(const uint8_t *f, uint32_t len, uint32_t at)
{
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) v = (v << 8) | (at + k < len ? f[at + k] : 0u);
    return v;
}

}  // namespace

extern "C" int rxg_flow_trains_host(const void *recs, uint32_t rec_kind, void *const *frames, const uint16_t *len,
                                    uint32_t n, uint32_t ntcb, uint32_t flags, const uint32_t *cur_seq,
                                    uint32_t *order, uint64_t cap_seg, rxg_flow_train *trains, uint64_t cap_trains,
                                    uint64_t count[4])
{
    if (!count || (n && !recs) || (cap_seg && !order) || (cap_trains && !trains)) return -EINVAL;
    if (rec_kind != RXG_REC8 && rec_kind != RXG_REC16 && rec_kind != RXG_REC48) return -EINVAL;
    if (n && rec_kind != RXG_REC48 && (!frames || !len)) return -EINVAL;
    if (ntcb == 0 || ntcb > RXG_FS_MAX_NTCB || (flags & ~RXG_FT_TCP_OK_ONLY)) return -EINVAL;
    count[0] = count[1] = count[2] = count[3] = 0;
    if (!n) return 0;
    std::vector<Seg> segs;
    try {
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t *r = (const uint8_t *)recs + (size_t)i * rec_kind;
            rxg_rec16 c;
            if (rec_kind == RXG_REC8) rxg_rec8_expand((const rxg_rec8 *)r, &c);
            else c = *(const rxg_rec16 *)r;
            if (c.verdict != RXG_V_DISPATCH) continue;
            if (c.tcb_idx < 0 || (uint32_t)c.tcb_idx >= ntcb) {
                ++count[2];
                continue;
            }
            if ((flags & RXG_FT_TCP_OK_ONLY) && !(c.flags & RXG_F_TCP_OK)) {
                ++count[3];
                continue;
            }
            if (c.datalen <= 0 || c.datalen > 65535) continue;
            Seg s;
            s.tcb = c.tcb_idx;
            s.idx = i;
            s.seq = rec_kind == RXG_REC48 ? ((const rxg_rec48 *)r)->seq
                                          : be32_cut((const uint8_t *)frames[i], len[i], 38);
            s.datalen = (uint32_t)c.datalen;
            s.fin = (c.tcp_flags & 0x01u) != 0;
            segs.push_back(s);
        }
        // (already in packet order: a stable sort on tcb_idx alone is the rule's order)
        std::stable_sort(segs.begin(), segs.end(), [](const Seg &a, const Seg &b) { return a.tcb < b.tcb; });
    } catch (const std::bad_alloc &) {
        return -ENOMEM;
    }
    const uint64_t S = segs.size();
    count[0] = S;
    for (uint64_t k = 0; k < S && k < cap_seg; ++k) order[k] = segs[k].idx;
    uint64_t T = 0;
    for (uint64_t k = 0; k < S;) {
        uint64_t e = k + 1;
        while (e < S && segs[e].tcb == segs[k].tcb && segs[e].seq == (uint32_t)(segs[e - 1].seq + segs[e - 1].datalen) &&
               !segs[e - 1].fin && !segs[e - 1].wraps() && !segs[e].wraps())
            ++e;
        if (T < cap_trains) {
            const Seg &a = segs[k], &z = segs[e - 1];
            rxg_flow_train t;
            t.tcb_idx = a.tcb;
            t.first = (uint32_t)k;
            t.nseg = (uint32_t)(e - k);
            t.seq = a.seq;
            t.bytes = 0;
            for (uint64_t j = k; j < e; ++j) t.bytes += segs[j].datalen;
            t.next_ack = (uint32_t)(a.seq + t.bytes) + (z.fin ? 1u : 0u);
            const bool flow_first = k == 0 || segs[k - 1].tcb != a.tcb;
            const bool flow_last = e == S || segs[e].tcb != a.tcb;
            t.flags = (z.fin ? RXG_FTR_FIN : 0u) | (a.wraps() ? RXG_FTR_WRAP : 0u) |
                      (flow_first ? RXG_FTR_FLOW_FIRST : 0u) | (flow_last ? RXG_FTR_FLOW_LAST : 0u);
            if (flow_first && cur_seq && cur_seq[a.tcb] != 0 && cur_seq[a.tcb] == a.seq && !a.wraps())
                t.flags |= RXG_FTR_HEAD;
            trains[T] = t;
        }
        ++T;
        k = e;
    }
    count[1] = T;
    return 0;
}
