// rxg_flowsum.cpp — rxg_flow_sums_host: the per-flow summary rule of rxg.h applied to a burst in
// host memory (rxg_rx_burst's records and the caller's frames), without a context or a GPU.
// The device form is rxg_flowsum.hip.
#include <cerrno>
#include <cstddef>
#include <cstdlib>
#include <algorithm>
#include <new>
#include <vector>

#include "rxg.h"

static_assert(sizeof(rxg_flow_sum) == 40 && offsetof(rxg_flow_sum, tcp_flags_or) == 28 &&
                  offsetof(rxg_flow_sum, data_bytes) == 32,
              "rxg_flow_sum layout");

namespace {

// big-endian frame[at .. at + 4), bytes at or beyond len read as zero
inline uint32_t be32_cut(const uint8_t *f, uint32_t len, uint32_t at)
{
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) v = (v << 8) | (at + k < len ? f[at + k] : 0u);
    return v;
}

}  // namespace

extern "C" int rxg_flow_sums_host(const void *recs, uint32_t rec_kind, void *const *frames, const uint16_t *len,
                                  uint32_t n, uint32_t ntcb, uint32_t flags, rxg_flow_sum *out, uint64_t cap,
                                  uint64_t count[3])
{
    if (!count || (n && !recs) || (cap && !out)) return -EINVAL;
    if (rec_kind != RXG_REC8 && rec_kind != RXG_REC16 && rec_kind != RXG_REC48) return -EINVAL;
    if (n && rec_kind != RXG_REC48 && (!frames || !len)) return -EINVAL;
    if (ntcb == 0 || ntcb > RXG_FS_MAX_NTCB || (flags & ~RXG_FS_TCP_OK_ONLY)) return -EINVAL;
    count[0] = count[1] = count[2] = 0;
    if (!n) return 0;
    // a dense accumulator (zero pages until touched) and the flows in the order they appear
    rxg_flow_sum *acc = (rxg_flow_sum *)std::calloc(ntcb, sizeof(rxg_flow_sum));
    if (!acc) return -ENOMEM;
    std::vector<int32_t> seen;
    try {
        for (uint32_t i = 0; i < n; ++i) {
            const uint8_t *r = (const uint8_t *)recs + (size_t)i * rec_kind;
            rxg_rec16 c;
            if (rec_kind == RXG_REC8) rxg_rec8_expand((const rxg_rec8 *)r, &c);
            else c = *(const rxg_rec16 *)r;
            if (c.verdict != RXG_V_DISPATCH) continue;
            if (c.tcb_idx < 0 || (uint32_t)c.tcb_idx >= ntcb) {
                ++count[1];
                continue;
            }
            if ((flags & RXG_FS_TCP_OK_ONLY) && !(c.flags & RXG_F_TCP_OK)) {
                ++count[2];
                continue;
            }
            uint32_t seq, ack;
            if (rec_kind == RXG_REC48) {
                seq = ((const rxg_rec48 *)r)->seq;
                ack = ((const rxg_rec48 *)r)->ack;
            } else {
                const uint8_t *f = (const uint8_t *)frames[i];
                seq = be32_cut(f, len[i], 38);
                ack = be32_cut(f, len[i], 42);
            }
            rxg_flow_sum &s = acc[c.tcb_idx];
            if (!s.frames) {
                seen.push_back(c.tcb_idx);
                s.tcb_idx = c.tcb_idx;
                s.first_idx = i;
                s.state = c.state;
            }
            ++s.frames;
            s.max_seq = std::max(s.max_seq, seq);
            s.max_ack = std::max(s.max_ack, ack);
            s.last_idx = i;
            s.tcp_flags_or |= c.tcp_flags;
            if (c.datalen > 0) {
                ++s.data_frames;
                s.data_bytes += (uint64_t)c.datalen;
            }
        }
        std::sort(seen.begin(), seen.end());
    } catch (const std::bad_alloc &) {
        std::free(acc);
        return -ENOMEM;
    }
    count[0] = seen.size();
    for (uint64_t k = 0; k < seen.size() && k < cap; ++k) out[k] = acc[seen[k]];
    std::free(acc);
    return 0;
}
