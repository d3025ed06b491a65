// rxopt_check.cpp — rxg_rx_opt_parse stand-alone (tests/test_rxopt_host.py builds this with
// csrc/rxg_rxopt.cpp, plain and under ASan/UBSan).  Every frame is copied to a heap block of
// exactly `len` bytes and parsed there, so a read at or beyond len is a heap overflow the
// sanitizer reports; the records are checked against answers worked out by hand, and against a
// parse of the same bytes in a large zero-padded buffer (bytes beyond len read as zero).
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rxg.h"

static int failures = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAIL line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// 54 header bytes with data_off d, then opts
static std::vector<uint8_t> frame_of(unsigned d, const std::vector<uint8_t> &opts, size_t extra = 0)
{
    std::vector<uint8_t> f(54, 0);
    f[12] = 0x08;
    f[14] = 0x45;
    f[23] = 6;
    f[46] = (uint8_t)(d << 4);
    f.insert(f.end(), opts.begin(), opts.end());
    f.insert(f.end(), extra, (uint8_t)0x08);  // payload that would parse as a timestamp's kind
    return f;
}

static rxg_rx_opt parse_exact(const std::vector<uint8_t> &f, size_t len)
{
    uint8_t *blk = len ? (uint8_t *)malloc(len) : nullptr;  // flush against the block's end
    if (len) memcpy(blk, f.data(), len);
    rxg_rx_opt o;
    memset(&o, 0xA5, sizeof o);
    CHECK(rxg_rx_opt_parse(blk, (uint32_t)len, &o) == 0);
    free(blk);
    return o;
}

int main()
{
    static_assert(sizeof(rxg_rx_opt) == 16, "record size");
    // the common SYN
    const std::vector<uint8_t> syn = {2, 4, 5, 0xb4, 4, 2, 8, 10, 0, 0, 0x12, 0x34, 0, 0, 0, 0, 1, 3, 3, 7};
    rxg_rx_opt o = parse_exact(frame_of(10, syn), 74);
    CHECK(o.mss == 1460 && o.wscale == 7 && o.tsval == 0x1234 && o.tsecr == 0 && o.nsack == 0 && o.sack_off == 0);
    CHECK(o.opt_len == 20 && o.flags == (RXG_O_PARSED | RXG_O_MSS | RXG_O_WSCALE | RXG_O_SACK_PERM | RXG_O_TS));
    // a SACK of two blocks behind two no-operations
    std::vector<uint8_t> sk = {1, 1, 5, 18};
    sk.resize(20, 0x11);
    o = parse_exact(frame_of(10, sk), 74);
    CHECK(o.nsack == 2 && o.sack_off == 58 && o.flags == (RXG_O_PARSED | RXG_O_SACK) && o.opt_len == 20);
    // data_off below 5
    o = parse_exact(frame_of(4, syn), 74);
    CHECK(o.flags == (RXG_O_PARSED | RXG_O_BAD_DOFF) && o.opt_len == 0 && o.mss == 0);

    // every length of a frame that claims 40 option bytes, all of them options when whole: the
    // exact-size parse equals the parse of the zero-padded copy, and CUT is set below 94
    std::vector<uint8_t> full = {8, 10, 1, 2, 3, 4, 5, 6, 7, 8, 2, 4, 5, 0xb4, 5, 10, 9, 9, 9, 9, 8, 8, 8, 8,
                                 3, 3, 9, 4, 2, 8, 10, 0, 0, 0, 5, 0, 0, 0, 6, 1};
    CHECK(full.size() == 40);
    const std::vector<uint8_t> whole = frame_of(15, full, 30);
    for (size_t len = 0; len <= whole.size(); ++len) {
        const rxg_rx_opt a = parse_exact(whole, len);
        std::vector<uint8_t> padded(whole.begin(), whole.begin() + (long)len);
        padded.resize(256, 0);
        rxg_rx_opt b;
        CHECK(rxg_rx_opt_parse(padded.data(), 256, &b) == 0);
        const bool cut = len < 94 && len > 46;  // below 47 data_off itself reads zero: O = 0
        b.flags = (uint16_t)((b.flags & ~RXG_O_CUT) | (len < 54 || cut ? RXG_O_CUT : 0));
        CHECK(memcmp(&a, &b, sizeof a) == 0);
        CHECK(((a.flags & RXG_O_CUT) != 0) == (len < 54 || cut));
        if (len <= 46) CHECK(a.flags == (RXG_O_PARSED | RXG_O_BAD_DOFF | RXG_O_CUT) && a.opt_len == 0);
        if (len >= 94) CHECK(a.tsval == 5 && a.tsecr == 6 && a.mss == 1460 && a.wscale == 9 && a.nsack == 1 && a.sack_off == 70);
    }
    // malformed forms, each at the very end of its block
    o = parse_exact(frame_of(6, {2, 0, 5, 0xb4}), 58);
    CHECK(o.flags == (RXG_O_PARSED | RXG_O_MALFORMED));
    o = parse_exact(frame_of(6, {1, 1, 1, 8}), 58);
    CHECK(o.flags == (RXG_O_PARSED | RXG_O_MALFORMED));
    o = parse_exact(frame_of(6, {1, 1, 8, 10}), 58);
    CHECK(o.flags == (RXG_O_PARSED | RXG_O_MALFORMED) && o.tsval == 0);
    o = parse_exact(frame_of(6, {254, 4, 1, 1}), 58);
    CHECK(o.flags == (RXG_O_PARSED | RXG_O_OTHER));
    // argument errors
    rxg_rx_opt z;
    CHECK(rxg_rx_opt_parse(whole.data(), 10, nullptr) == -EINVAL);
    CHECK(rxg_rx_opt_parse(nullptr, 1, &z) == -EINVAL);
    CHECK(rxg_rx_opt_parse(nullptr, 0, &z) == 0 && z.flags == (RXG_O_PARSED | RXG_O_BAD_DOFF | RXG_O_CUT));
    if (failures) return 1;
    printf("rxopt ok\n");
    return 0;
}
