// rxg_trainpay.cpp — rxg_train_payload_host: the train-payload rule of rxg.h applied to a burst
// in host memory, without a context or a GPU.  The device form is rxg_trainpay.hip.
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstring>

#include "rxg.h"

static_assert(sizeof(rxg_payload_msg) == 16 && sizeof(rxg_dev_train_payload) == 136 &&
                  offsetof(rxg_dev_train_payload, arena) == 96 && offsetof(rxg_dev_train_payload, arena_used) == 128,
              "train payload layouts");

namespace {

inline uint64_t pad16(uint64_t b) { return (b + 15u) & ~(uint64_t)15u; }

}  // namespace

extern "C" int rxg_train_payload_host(const void *recs, uint32_t rec_kind, void *const *frames, const uint16_t *len,
                                      uint32_t n, const uint32_t *order, uint64_t cap_seg, const rxg_flow_train *trains,
                                      uint64_t cap_trains, const uint64_t count[4], uint32_t flags, void *arena,
                                      uint64_t arena_cap, rxg_payload_msg *msgs, rxg_payload_msg *tmsgs,
                                      uint64_t *arena_used)
{
    if (!count || !arena_used || (n && (!recs || !frames || !len)) || (cap_seg && !order) || (cap_trains && !trains) ||
        (arena_cap && !arena))
        return -EINVAL;
    if (rec_kind != RXG_REC8 && rec_kind != RXG_REC16 && rec_kind != RXG_REC48) return -EINVAL;
    if (flags & ~RXG_TP_HEAD_ONLY) return -EINVAL;
    *arena_used = 0;
    if (!n) return 0;
    if (msgs) std::memset(msgs, 0, (size_t)n * sizeof *msgs);
    const uint64_t S = std::min(std::min(count[0], cap_seg), (uint64_t)n);
    const uint64_t T = S == 0 ? 0 : std::min(std::min(count[1], cap_trains), (uint64_t)n);
    uint64_t at = 0;
    for (uint64_t k = 0; k < T; ++k) {
        const rxg_flow_train &t = trains[k];
        rxg_payload_msg tm = {0, 0, 0};
        const bool takes = (uint64_t)t.first + t.nseg <= S && t.bytes <= 0xFFFFFFFFull &&
                           (!(flags & RXG_TP_HEAD_ONLY) || (t.flags & RXG_FTR_HEAD));
        if (takes) {
            const uint64_t off = at, span = pad16(t.bytes);
            at += span;
            if (off + span <= arena_cap) {
                uint8_t *dst = (uint8_t *)arena + off;
                tm.arena_off = off;
                tm.len = (uint32_t)t.bytes;
                tm.flags = RXG_PM_GATHERED;
                for (uint32_t j = 0; j < t.nseg; ++j) {
                    const uint32_t i = order[(uint64_t)t.first + j];
                    bool copied = false;
                    if (i < n) {
                        const uint8_t *r = (const uint8_t *)recs + (size_t)i * rec_kind;
                        rxg_rec16 c;
                        if (rec_kind == RXG_REC8) rxg_rec8_expand((const rxg_rec8 *)r, &c);
                        else std::memcpy(&c, r, sizeof c);
                        const uint8_t *f = (const uint8_t *)frames[i];
                        const uint32_t flen = len[i];
                        if (c.verdict <= RXG_V_RST_LISTEN_NONSYN && c.datalen > 0 && !(c.flags & RXG_F_TRUNC) && flen > 46) {
                            const uint32_t start = 34u + (uint32_t)(f[46] >> 4) * 4u, dl = (uint32_t)c.datalen;
                            uint32_t seq;
                            if (rec_kind == RXG_REC48) seq = ((const rxg_rec48 *)r)->seq;
                            else seq = (uint32_t)f[38] << 24 | (uint32_t)f[39] << 16 | (uint32_t)f[40] << 8 | f[41];
                            const uint32_t rel = seq - t.seq;
                            if ((uint64_t)start + dl <= flen && (uint64_t)rel + dl <= t.bytes) {
                                std::memcpy(dst + rel, f + start, dl);
                                if (msgs) {
                                    msgs[i].arena_off = off + rel;
                                    msgs[i].len = dl;
                                    msgs[i].flags = (uint32_t)RXG_PM_GATHERED |
                                                    (dl >= 1000u ? (uint32_t)RXG_PM_REF_OVERSIZE : 0u);
                                }
                                copied = true;
                            }
                        }
                    }
                    if (!copied) tm.flags |= RXG_PM_HOLE;
                }
                std::memset(dst + t.bytes, 0, (size_t)(span - t.bytes));
            }
        }
        if (tmsgs) tmsgs[k] = tm;
    }
    *arena_used = at;
    return 0;
}
