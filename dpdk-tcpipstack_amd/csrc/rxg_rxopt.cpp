// rxg_rxopt.cpp — rxg_rx_opt_parse: the received-option rule of rxg.h applied to one frame on
// the host, for frames that reach the stack outside a burst's option pass (rxg_rx_opts_dev,
// rxg_rxopt.hip).  Pure host code (rxg.h and libc only: it compiles stand-alone).
#include <errno.h>
#include <stddef.h>
#include <string.h>

#include "rxg.h"

static_assert(sizeof(rxg_rx_opt) == 16 && offsetof(rxg_rx_opt, mss) == 8 && offsetof(rxg_rx_opt, flags) == 14,
              "received-option record layout");

extern "C" int rxg_rx_opt_parse(const uint8_t *frame, uint32_t len, rxg_rx_opt *out)
{
    if (!out || (!frame && len)) return -EINVAL;
    memset(out, 0, sizeof *out);
    uint32_t flags = RXG_O_PARSED;
    const uint32_t d = len > 46u ? (uint32_t)(frame[46] >> 4) : 0u;  // bytes at and beyond len read as zero
    uint32_t O = 0;
    if (d < 5u) flags |= RXG_O_BAD_DOFF;
    else O = 4u * d - 20u;
    if (54u + O > len) flags |= RXG_O_CUT;
    uint8_t b[40];
    for (uint32_t j = 0; j < O; ++j) b[j] = 54u + j < len ? frame[54u + j] : (uint8_t)0;
    uint32_t p = 0;
    while (p < O) {
        const uint32_t k = b[p];
        if (k == 0u) break;
        if (k == 1u) {
            ++p;
            continue;
        }
        if (p + 1u >= O) {
            flags |= RXG_O_MALFORMED;
            break;
        }
        const uint32_t l = b[p + 1u];
        if (l < 2u || p + l > O) {
            flags |= RXG_O_MALFORMED;
            break;
        }
        const uint8_t *v = b + p + 2u;
        if (k == 2u && l == 4u) {
            out->mss = (uint16_t)((v[0] << 8) | v[1]);
            flags |= RXG_O_MSS;
        } else if (k == 3u && l == 3u) {
            out->wscale = v[0];
            flags |= RXG_O_WSCALE;
        } else if (k == 4u && l == 2u) {
            flags |= RXG_O_SACK_PERM;
        } else if (k == 5u && (l == 10u || l == 18u || l == 26u || l == 34u)) {
            out->nsack = (uint8_t)((l - 2u) / 8u);
            out->sack_off = (uint8_t)(54u + p + 2u);
            flags |= RXG_O_SACK;
        } else if (k == 8u && l == 10u) {
            out->tsval = ((uint32_t)v[0] << 24) | ((uint32_t)v[1] << 16) | ((uint32_t)v[2] << 8) | v[3];
            out->tsecr = ((uint32_t)v[4] << 24) | ((uint32_t)v[5] << 16) | ((uint32_t)v[6] << 8) | v[7];
            flags |= RXG_O_TS;
        } else {
            flags |= RXG_O_OTHER;
        }
        p += l;
    }
    out->opt_len = (uint8_t)O;
    out->flags = (uint16_t)flags;
    return 0;
}
