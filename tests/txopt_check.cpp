// txopt_check.cpp — the option helpers and rxg_tx_plan_opt (dpdk-tcpipstack_amd/csrc/
// rxg_txopt.cpp, with rxg_txplan.cpp) driven stand-alone: the helpers' bytes, the planner's
// error cases, and 5 000 random batches each checked against rxg_tx_plan run send by send at
// mss - O, with heap buffers of exactly the size asked for so that a write past `cap`, or a
// read past the block table, is out of bounds (built under ASan/UBSan by the test).
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

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd()
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void helpers()
{
    for (uint32_t n = 0; n <= 40; ++n) {
        // a source of exactly n bytes and a block on the heap: nothing past either is touched
        uint8_t *src = (uint8_t *)malloc(n ? n : 1);
        for (uint32_t i = 0; i < n; ++i) src[i] = (uint8_t)(i + 1);
        rxg_tx_opt *o = (rxg_tx_opt *)malloc(sizeof(rxg_tx_opt));
        memset(o, 0xEE, sizeof *o);
        const int rc = rxg_tx_opt_set(o, n ? src : nullptr, n);
        CHECK(rc == (int)((n + 3) / 4 * 4) && o->len == rc);
        uint8_t want[48];
        memset(want, 0, sizeof want);
        want[0] = (uint8_t)rc;
        memcpy(want + 6, src, n);
        CHECK(memcmp(o, want, 48) == 0);
        free(o);
        free(src);
    }
    rxg_tx_opt o;
    uint8_t big[41] = {0};
    CHECK(rxg_tx_opt_set(&o, big, 41) == -EINVAL);
    CHECK(rxg_tx_opt_set(nullptr, big, 4) == -EINVAL);
    CHECK(rxg_tx_opt_set(&o, nullptr, 4) == -EINVAL);
    CHECK(rxg_tx_opt_timestamp(nullptr, 1, 2) == -EINVAL);
    CHECK(rxg_tx_opt_ref_ack(nullptr) == -EINVAL);
    CHECK(rxg_tx_opt_timestamp(&o, 0x01020304u, 0xA0B0C0D0u) == 12 && o.len == 12);
    const uint8_t ts[12] = {1, 1, 8, 10, 1, 2, 3, 4, 0xA0, 0xB0, 0xC0, 0xD0};
    CHECK(memcmp(o.bytes, ts, 12) == 0);
    CHECK(rxg_tx_opt_ref_ack(&o) == 20 && o.len == 20);
    const uint8_t ack[20] = {8, 10, 0x18, 0x19, 0x03, 0, 0, 0, 0, 0, 2, 4, 0x05, 0x14, 3, 3, 7, 0, 0, 0};
    CHECK(memcmp(o.bytes, ack, 20) == 0);
    for (int i = 20; i < 40; ++i) CHECK(o.bytes[i] == 0);
}

static void one_batch(const std::vector<rxg_tx_send> &sends, const std::vector<uint32_t> &send_opt,
                      const std::vector<rxg_tx_opt> &table, uint32_t mss)
{
    // heap copies of exactly the sizes passed
    const uint32_t nopts = (uint32_t)table.size();
    rxg_tx_opt *opts = (rxg_tx_opt *)malloc(nopts ? nopts * sizeof(rxg_tx_opt) : 1);
    if (nopts) memcpy(opts, table.data(), nopts * sizeof(rxg_tx_opt));
    std::vector<rxg_tx_seg> want;
    std::vector<uint32_t> want_next(sends.size());
    for (size_t j = 0; j < sends.size(); ++j) {
        const uint32_t O = send_opt[j] ? table[send_opt[j] - 1].len : 0;
        const uint32_t m = mss - O;
        const uint32_t nseg = sends[j].bytes ? (uint32_t)(((uint64_t)sends[j].bytes + m - 1) / m) : 1;
        std::vector<rxg_tx_seg> v(nseg);
        CHECK(rxg_tx_plan(&sends[j], 1, m, v.data(), nseg, &want_next[j]) == (int64_t)nseg);
        for (rxg_tx_seg &s : v) {
            s.reserved = send_opt[j];
            CHECK(s.data_len <= m);
        }
        want.insert(want.end(), v.begin(), v.end());
    }
    const uint64_t cap = want.size();
    rxg_tx_seg *out = (rxg_tx_seg *)malloc(cap ? cap * sizeof(rxg_tx_seg) : 1);
    uint32_t *next = (uint32_t *)malloc(sends.size() * sizeof(uint32_t) + 1);
    const int64_t n = rxg_tx_plan_opt(sends.data(), (uint32_t)sends.size(), mss, send_opt.data(), opts, nopts, out, cap, next);
    CHECK(n == (int64_t)cap);
    if (n == (int64_t)cap && cap) {
        CHECK(memcmp(out, want.data(), cap * sizeof(rxg_tx_seg)) == 0);
        CHECK(memcmp(next, want_next.data(), sends.size() * sizeof(uint32_t)) == 0);
    }
    free(out);
    free(next);
    if (cap) {
        rxg_tx_seg *small = (rxg_tx_seg *)malloc((cap - 1) * sizeof(rxg_tx_seg) + 1);
        CHECK(rxg_tx_plan_opt(sends.data(), (uint32_t)sends.size(), mss, send_opt.data(), opts, nopts, small, cap - 1,
                              nullptr) == -ENOSPC);
        free(small);
    }
    free(opts);
}

static rxg_tx_send random_send(uint32_t mss)
{
    rxg_tx_send s;
    memset(&s, 0, sizeof s);
    s.flow = (uint32_t)rnd();
    s.next_seq = (uint32_t)rnd();
    s.ack = (uint32_t)rnd();
    s.src_off = rnd() >> 8;
    s.bytes = (uint32_t)(rnd() % (6 * mss + 3));
    s.tcp_flags = (uint8_t)rnd();
    s.win_raw = (uint16_t)rnd();
    s.ip_id0 = (uint16_t)rnd();
    return s;
}

int main()
{
    helpers();
    std::vector<rxg_tx_opt> table(11);
    for (uint32_t k = 0; k < table.size(); ++k) {  // lengths 0, 4, .. 40, garbage everywhere else
        for (size_t i = 0; i < sizeof(rxg_tx_opt); ++i) ((uint8_t *)&table[k])[i] = (uint8_t)rnd();
        table[k].len = (uint8_t)(4 * k);
    }
    for (int i = 0; i < 5000; ++i) {
        const uint32_t mss = 41 + (uint32_t)(rnd() % 3000);
        const uint32_t nsends = (uint32_t)(rnd() % 6);
        const uint32_t nopts = (uint32_t)(rnd() % (table.size() + 1));
        std::vector<rxg_tx_send> sends;
        std::vector<uint32_t> send_opt;
        for (uint32_t j = 0; j < nsends; ++j) {
            sends.push_back(random_send(mss));
            send_opt.push_back((uint32_t)(rnd() % (nopts + 1)));
        }
        one_batch(sends, send_opt, std::vector<rxg_tx_opt>(table.begin(), table.begin() + nopts), mss);
    }
    {   // send_opt NULL: rxg_tx_plan's output, the table not looked at
        std::vector<rxg_tx_send> sends;
        for (int j = 0; j < 7; ++j) sends.push_back(random_send(1460));
        std::vector<rxg_tx_seg> a(64), b(64);
        std::vector<uint32_t> na(7), nb(7);
        memset(a.data(), 0xEE, 64 * sizeof(rxg_tx_seg));
        memset(b.data(), 0xEE, 64 * sizeof(rxg_tx_seg));
        const int64_t n = rxg_tx_plan(sends.data(), 7, 1460, a.data(), 64, na.data());
        CHECK(n > 0 && rxg_tx_plan_opt(sends.data(), 7, 1460, nullptr, nullptr, 5, b.data(), 64, nb.data()) == n);
        CHECK(memcmp(a.data(), b.data(), 64 * sizeof(rxg_tx_seg)) == 0 && na == nb);
    }
    {   // errors: nothing is written
        rxg_tx_send two[2] = {random_send(1000), random_send(1000)};
        rxg_tx_opt bad[4];
        memset(bad, 0, sizeof bad);
        bad[0].len = 12;
        bad[1].len = 44;
        bad[2].len = 6;
        bad[3].len = 40;
        rxg_tx_seg *out = (rxg_tx_seg *)malloc(32 * sizeof(rxg_tx_seg));
        memset(out, 0xEE, 32 * sizeof(rxg_tx_seg));
        const uint32_t cases[][3] = {{5, 4, 1460}, {2, 4, 1460}, {3, 4, 1460}, {1, 0, 1460}, {1, 4, 12}, {4, 4, 40},
                                     {0, 4, 0}, {0, 4, RXG_TX_MAX_DATA + 1}};
        for (const auto &c : cases) {
            const uint32_t so[2] = {0, c[0]};
            CHECK(rxg_tx_plan_opt(two, 2, c[2], so, bad, c[1], out, 32, nullptr) == -EINVAL);
        }
        const uint32_t so[2] = {0, 1};
        CHECK(rxg_tx_plan_opt(two, 2, 1460, so, nullptr, 4, out, 32, nullptr) == -EINVAL);
        CHECK(rxg_tx_plan_opt(nullptr, 2, 1460, so, bad, 4, out, 32, nullptr) == -EINVAL);
        CHECK(rxg_tx_plan_opt(two, 2, 1460, so, bad, 4, nullptr, 32, nullptr) == -EINVAL);
        for (size_t i = 0; i < 32 * sizeof(rxg_tx_seg); ++i) CHECK(((uint8_t *)out)[i] == 0xEE);
        free(out);
    }
    if (fails) return 1;
    printf("txopt ok\n");
    return 0;
}
