// rxg_ackplan.cpp — rxg_ack_plan_host: the ACK-plan rule of rxg.h applied to host arrays, without a
// context or a GPU.  The device form is rxg_ackplan.hip.
#include <algorithm>
#include <cerrno>
#include <cstddef>
#include <cstring>

#include "rxg.h"

static_assert(sizeof(rxg_ack_state) == 16 && sizeof(rxg_ack) == 16 && sizeof(rxg_dev_ack_plan) == 128 &&
                  offsetof(rxg_dev_ack_plan, state) == 56 && offsetof(rxg_dev_ack_plan, opts) == 88 &&
                  offsetof(rxg_dev_ack_plan, count) == 120,
              "ACK plan layouts");

extern "C" int rxg_ack_plan_host(const rxg_dev_ack_plan *p)
{
    if (!p || !p->train_count || !p->state || !p->count || (p->cap_seg && !p->order) ||
        (p->cap_trains && !p->trains) || (p->cap && (!p->segs || !p->acks)))
        return -EINVAL;
    if (p->opt_plain > p->opt_base || p->opt_base > p->opt_cap) return -EINVAL;
    if (p->ntcb == 0 || p->ntcb > RXG_FS_MAX_NTCB || p->flags) return -EINVAL;
    uint64_t *count = p->count;
    count[0] = count[1] = count[2] = count[3] = 0;
    const uint64_t n = p->n;
    const uint64_t S = std::min(std::min(p->train_count[0], p->cap_seg), n);
    const uint64_t T = S == 0 ? 0 : std::min(std::min(p->train_count[1], p->cap_trains), n);
    uint64_t a = 0;
    for (uint64_t k = 0; k < T; ++k) {
        const rxg_flow_train &t = p->trains[k];
        if (k && p->trains[k - 1].tcb_idx == t.tcb_idx) continue;  // not its flow's first train
        if (t.tcb_idx < 0 || (uint32_t)t.tcb_idx >= p->ntcb) {
            ++count[2];
            continue;
        }
        const rxg_ack_state &s = p->state[t.tcb_idx];
        if (!(s.flags & RXG_AS_LIVE)) {
            ++count[1];
            continue;
        }
        const bool adv = (t.flags & RXG_FTR_HEAD) != 0;
        uint32_t fl = adv ? (uint32_t)RXG_ACK_ADVANCES | ((t.flags & RXG_FTR_FIN) ? (uint32_t)RXG_ACK_FIN : 0u)
                          : (uint32_t)RXG_ACK_DUP;
        const uint32_t ack = adv ? t.next_ack : s.rcv_ack;
        uint32_t reserved = p->opt_plain;
        if ((s.flags & RXG_AS_TS) && p->opts) {
            if ((uint64_t)p->opt_base + a < p->opt_cap) {
                uint32_t tsecr = s.ts_recent;
                if (adv && p->rxopts && t.first < S) {
                    const uint32_t pkt = p->order[t.first];
                    if (pkt < n && (p->rxopts[pkt].flags & RXG_O_TS)) tsecr = p->rxopts[pkt].tsval;
                }
                reserved = (uint32_t)(p->opt_base + a + 1u);
                if (a < p->cap) rxg_tx_opt_timestamp(&p->opts[p->opt_base + a], p->tsval_now, tsecr);
            } else {
                fl |= RXG_ACK_NO_OPT;
                ++count[3];
            }
        }
        if (a < p->cap) {
            rxg_tx_seg g;
            std::memset(&g, 0, sizeof g);
            g.flow = (uint32_t)t.tcb_idx;
            g.seq = s.snd_nxt;
            g.ack = ack;
            g.win_raw = s.win_raw;
            g.ip_id = (uint16_t)(p->ip_id0 + a);
            g.tcp_flags = RXG_TCP_FLAG_ACK;
            g.reserved = reserved;
            p->segs[a] = g;
            rxg_ack r;
            r.tcb_idx = t.tcb_idx;
            r.ack = ack;
            r.seq = s.snd_nxt;
            r.flags_train = fl | ((uint32_t)k << 8);
            p->acks[a] = r;
        }
        ++a;
    }
    count[0] = a;
    return 0;
}
