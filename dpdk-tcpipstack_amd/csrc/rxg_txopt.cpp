// rxg_txopt.cpp — the host side of TCP option blocks (rxg_tx_build_opt_dev's table entries):
// rxg_tx_opt_set / _timestamp / _ref_ack fill a block, rxg_tx_plan_opt cuts sends whose
// segments carry one, rxg_tx_plan_count counts the segments of such a cut (the `n` of the build
// that follows rxg_tx_plan_dev).  Pure host code (rxg.h, rxg_tx_plan and libc only: it compiles
// stand-alone with rxg_txplan.cpp).
#include <errno.h>
#include <stddef.h>
#include <string.h>

#include "rxg.h"

static_assert(sizeof(rxg_tx_opt) == 48 && offsetof(rxg_tx_opt, bytes) == 6, "option block layout");

extern "C" int rxg_tx_opt_set(rxg_tx_opt *o, const uint8_t *bytes, uint32_t n)
{
    if (!o || n > 40u || (!bytes && n)) return -EINVAL;
    memset(o, 0, sizeof *o);  // the pad is kind 0, end of option list (tcp_out.c:262)
    if (n) memcpy(o->bytes, bytes, n);
    o->len = (uint8_t)((n + 3u) & ~3u);
    return o->len;
}

static void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

extern "C" int rxg_tx_opt_timestamp(rxg_tx_opt *o, uint32_t tsval, uint32_t tsecr)
{
    uint8_t b[12] = {1, 1, 8, 10};  // NOP NOP kind 8 len 10 (RFC 7323 appendix A)
    put_be32(b + 4, tsval);
    put_be32(b + 8, tsecr);
    return rxg_tx_opt_set(o, b, sizeof b);
}

extern "C" int rxg_tx_opt_ref_ack(rxg_tx_opt *o)
{
    // tcp_out.c:255: add_winscale_option(7) + add_mss_option(1300) + add_timestamp_option(203032,
    // 0), evaluated left to right (gcc), each prepending: in the frame the timestamp comes
    // first.  value and echo are stored as the host holds them (203032 = 0x00031918, x86).
    static const uint8_t b[17] = {8, 10, 0x18, 0x19, 0x03, 0x00, 0, 0, 0, 0,  // tcp_out.c:66-74
                                  2, 4, 0x05, 0x14,                           // htons(1300), tcp_out.c:20-27
                                  3, 3, 7};                                   // tcp_out.c:29-36
    return rxg_tx_opt_set(o, b, sizeof b);  // + 3 bytes of pad (tcp_out.c:258-262)
}

extern "C" int64_t rxg_tx_plan_count(const rxg_tx_send *sends, uint32_t nsends, uint32_t mss,
                                     const uint32_t *send_opt, const rxg_tx_opt *opts, uint32_t nopts)
{
    if (mss == 0 || mss > RXG_TX_MAX_DATA) return -EINVAL;
    if (nsends && !sends) return -EINVAL;
    uint64_t total = 0;
    for (uint32_t j = 0; j < nsends; ++j) {
        uint32_t O = 0;
        if (send_opt && send_opt[j]) {  // the planner's checks of a named block
            const uint32_t k = send_opt[j];
            if (k > nopts || !opts) return -EINVAL;
            O = opts[k - 1u].len;
            if (O > 40u || (O & 3u) || mss <= O) return -EINVAL;
        }
        const uint32_t m = mss - O;
        total += sends[j].bytes ? ((uint64_t)sends[j].bytes + m - 1u) / m : 1u;
    }
    return (int64_t)total;
}

extern "C" int64_t rxg_tx_plan_opt(const rxg_tx_send *sends, uint32_t nsends, uint32_t mss, const uint32_t *send_opt,
                                   const rxg_tx_opt *opts, uint32_t nopts, rxg_tx_seg *out, uint64_t cap,
                                   uint32_t *next_seq_out)
{
    if (!send_opt) return rxg_tx_plan(sends, nsends, mss, out, cap, next_seq_out);
    if (mss == 0 || mss > RXG_TX_MAX_DATA) return -EINVAL;
    if (nsends && (!sends || (!out && cap))) return -EINVAL;
    for (uint32_t j = 0; j < nsends; ++j) {  // every block named is checked before anything is written
        const uint32_t k = send_opt[j];
        if (k == 0) continue;
        if (k > nopts || !opts) return -EINVAL;
        const uint32_t O = opts[k - 1u].len;
        if (O > 40u || (O & 3u) || mss <= O) return -EINVAL;
    }
    uint64_t at = 0;
    for (uint32_t j = 0; j < nsends; ++j) {
        const uint32_t k = send_opt[j];
        const uint32_t O = k ? opts[k - 1u].len : 0u;
        // one send cut at mss - O by the planner itself (at <= cap)
        const int64_t got = rxg_tx_plan(sends + j, 1, mss - O, out ? out + at : out, cap - at,
                                        next_seq_out ? next_seq_out + j : next_seq_out);
        if (got < 0) return got;
        for (int64_t q = 0; q < got; ++q) out[at + (uint64_t)q].reserved = k;
        at += (uint64_t)got;
    }
    return (int64_t)at;
}
