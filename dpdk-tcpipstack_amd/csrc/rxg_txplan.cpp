// rxg_txplan.cpp — rxg_tx_plan: a batch of sends cut into the segment descriptors
// rxg_tx_build_dev takes.  Pure host code (rxg.h and libc only: it compiles stand-alone).
#include <errno.h>

#include "rxg.h"

extern "C" int64_t rxg_tx_plan(const rxg_tx_send *sends, uint32_t nsends, uint32_t mss, rxg_tx_seg *out,
                               uint64_t cap, uint32_t *next_seq_out)
{
    if (mss == 0 || mss > RXG_TX_MAX_DATA) return -EINVAL;
    if (nsends && (!sends || (!out && cap))) return -EINVAL;
    // flags carried by one segment of a send only
    const uint8_t first_only = RXG_TCP_FLAG_SYN, last_only = RXG_TCP_FLAG_FIN | RXG_TCP_FLAG_PSH;
    uint64_t k = 0;
    for (uint32_t j = 0; j < nsends; ++j) {
        const rxg_tx_send &s = sends[j];
        const uint32_t nseg = s.bytes ? (uint32_t)(((uint64_t)s.bytes + mss - 1u) / mss) : 1u;
        if (nseg > cap - k) return -ENOSPC;  // (k <= cap)
        uint32_t seq = s.next_seq, done = 0;
        uint16_t id = s.ip_id0;
        for (uint32_t q = 0; q < nseg; ++q) {
            const uint32_t len = s.bytes - done < mss ? s.bytes - done : mss;
            uint8_t fl = (uint8_t)(s.tcp_flags & ~(first_only | last_only));
            if (q == 0) fl |= s.tcp_flags & first_only;
            if (q == nseg - 1u) fl |= s.tcp_flags & last_only;
            rxg_tx_seg &o = out[k++];
            o.src_off = s.src_off + done;
            o.flow = s.flow;
            o.seq = seq;
            o.ack = s.ack;
            o.data_len = (uint16_t)len;
            o.win_raw = s.win_raw;
            o.ip_id = id++;
            o.tcp_flags = fl;
            o.pad = 0;
            o.reserved = 0;
            // ptcb->next_seq as tcp_out.c:176-185 advances it
            seq += len;
            if (fl & RXG_TCP_FLAG_SYN) seq += 1u;
            if (fl & RXG_TCP_FLAG_FIN) seq += 1u;
            done += len;
        }
        if (next_seq_out) next_seq_out[j] = seq;
    }
    return (int64_t)k;
}
