// txplan_check.cpp — rxg_tx_plan (dpdk-tcpipstack_amd/csrc/rxg_txplan.cpp) driven stand-alone:
// the edge cases of tests/test_txbuild_host.py and 10 000 random sends, each checked against a
// direct restatement of tcp_out.c:176-185, with output buffers of exactly the size asked for
// so that a write past `cap` is an out-of-bounds write (built under ASan/UBSan by the test).
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "rxg.h"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            ++fails;                                                  \
        }                                                             \
    } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The segments of one send, the slow way: one sendtcpdata call per segment.
static std::vector<rxg_tx_seg> expect(const rxg_tx_send &s, uint32_t mss, uint32_t *next_seq)
{
    std::vector<rxg_tx_seg> v;
    const uint32_t nseg = s.bytes ? (s.bytes + mss - 1) / mss : 1;
    uint32_t seq = s.next_seq, left = s.bytes;
    for (uint32_t q = 0; q < nseg; ++q) {
        rxg_tx_seg o;
        memset(&o, 0, sizeof o);
        const uint32_t len = left < mss ? left : mss;
        uint8_t fl = s.tcp_flags & (uint8_t)~(RXG_TCP_FLAG_SYN | RXG_TCP_FLAG_FIN | RXG_TCP_FLAG_PSH);
        if (q == 0) fl |= s.tcp_flags & RXG_TCP_FLAG_SYN;
        if (q + 1 == nseg) fl |= s.tcp_flags & (RXG_TCP_FLAG_FIN | RXG_TCP_FLAG_PSH);
        o.src_off = s.src_off + (s.bytes - left);
        o.flow = s.flow;
        o.seq = seq;                                    // sent_seq = next_seq       tcp_out.c:176
        o.ack = s.ack;
        o.data_len = (uint16_t)len;
        o.win_raw = s.win_raw;
        o.ip_id = (uint16_t)(s.ip_id0 + q);
        o.tcp_flags = fl;
        seq += len;                                     // next_seq += data_len      tcp_out.c:177
        if ((fl & RXG_TCP_FLAG_SYN) == RXG_TCP_FLAG_SYN) seq += 1;  //               tcp_out.c:178-181
        if ((fl & RXG_TCP_FLAG_FIN) == RXG_TCP_FLAG_FIN) seq += 1;  //               tcp_out.c:182-185
        left -= len;
        v.push_back(o);
    }
    *next_seq = seq;
    return v;
}

static void one_batch(const std::vector<rxg_tx_send> &sends, uint32_t mss)
{
    std::vector<rxg_tx_seg> want;
    std::vector<uint32_t> want_next(sends.size());
    for (size_t j = 0; j < sends.size(); ++j) {
        const std::vector<rxg_tx_seg> v = expect(sends[j], mss, &want_next[j]);
        want.insert(want.end(), v.begin(), v.end());
    }
    const uint64_t cap = want.size();
    // heap buffers of exactly cap (and cap - 1) entries: a write past them is reported
    rxg_tx_seg *out = (rxg_tx_seg *)malloc(cap * sizeof(rxg_tx_seg));
    uint32_t *next = (uint32_t *)malloc(sends.size() * sizeof(uint32_t) + 1);
    memset(out, 0xEE, cap * sizeof(rxg_tx_seg));
    const int64_t n = rxg_tx_plan(sends.data(), (uint32_t)sends.size(), mss, out, cap, next);
    CHECK(n == (int64_t)cap);
    if (n == (int64_t)cap && cap) {
        CHECK(memcmp(out, want.data(), cap * sizeof(rxg_tx_seg)) == 0);
        CHECK(memcmp(next, want_next.data(), sends.size() * sizeof(uint32_t)) == 0);
    }
    CHECK(rxg_tx_plan(sends.data(), (uint32_t)sends.size(), mss, out, cap, nullptr) == (int64_t)cap);
    free(out);
    free(next);
    if (cap) {
        rxg_tx_seg *small = (rxg_tx_seg *)malloc((cap - 1) * sizeof(rxg_tx_seg) + 1);
        CHECK(rxg_tx_plan(sends.data(), (uint32_t)sends.size(), mss, small, cap - 1, nullptr) == -ENOSPC);
        free(small);
    }
}

int main()
{
    const uint32_t mss = 1460;
    const uint32_t sizes[] = {0, 1, mss - 1, mss, mss + 1, 3 * mss, 3 * mss + 7};
    const uint8_t flags[] = {0, RXG_TCP_FLAG_SYN, RXG_TCP_FLAG_FIN, RXG_TCP_FLAG_SYN | RXG_TCP_FLAG_FIN,
                             RXG_TCP_FLAG_ACK | RXG_TCP_FLAG_PSH};
    std::vector<rxg_tx_send> all;
    for (uint32_t b : sizes)
        for (uint8_t f : flags) {
            rxg_tx_send s;
            memset(&s, 0, sizeof s);
            s.flow = 3;
            s.next_seq = 0xFFFFFF00u;  // wraps within the longer sends
            s.ack = 77;
            s.src_off = 12345;
            s.bytes = b;
            s.tcp_flags = f;
            s.win_raw = 0xFFFF;
            s.ip_id0 = 0xFFFE;
            one_batch({s}, mss);
            all.push_back(s);
        }
    one_batch(all, mss);
    one_batch({}, mss);
    CHECK(rxg_tx_plan(all.data(), 1, 0, nullptr, 0, nullptr) == -EINVAL);
    CHECK(rxg_tx_plan(all.data(), 1, RXG_TX_MAX_DATA + 1, nullptr, 0, nullptr) == -EINVAL);
    {   // the largest mss and a send of nearly 4 GiB's segment count (no output wanted: cap 0)
        rxg_tx_send s = all[0];
        s.bytes = 0xFFFFFFFFu;
        CHECK(rxg_tx_plan(&s, 1, RXG_TX_MAX_DATA, nullptr, 0, nullptr) == -ENOSPC);
    }
    std::vector<rxg_tx_send> batch;
    for (int i = 0; i < 10000; ++i) {
        rxg_tx_send s;
        memset(&s, 0, sizeof s);
        const uint32_t m = 1 + (uint32_t)(rnd() % 3000);
        s.flow = (uint32_t)rnd();
        s.next_seq = (uint32_t)rnd();
        s.ack = (uint32_t)rnd();
        s.src_off = rnd() >> 8;
        s.bytes = (uint32_t)(rnd() % (8 * m + 3));
        s.tcp_flags = (uint8_t)rnd();
        s.win_raw = (uint16_t)rnd();
        s.ip_id0 = (uint16_t)rnd();
        one_batch({s}, m);
        batch.push_back(s);
        if (batch.size() == 100) {
            one_batch(batch, 1 + (uint32_t)(rnd() % 65481));
            batch.clear();
        }
    }
    if (fails) return 1;
    printf("txplan ok\n");
    return 0;
}
