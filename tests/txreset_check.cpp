// txreset_check.cpp — rxg_reset_set_id (dpdk-tcpipstack_amd/csrc/rxg_txresetid.cpp) driven
// stand-alone: the ids of tests/test_txreset_host.py, a header whose sum folds to 0xFFFF
// (checksum 0x0000) and 100 000 random lines, each checked against a direct restatement of
// ip.c:44-59,102-107 on a copy.  Every line lives in a heap buffer of exactly 64 bytes, so a
// write outside it is an out-of-bounds write (the test builds this plain and under ASan/UBSan).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

// ip.c:44-59, as written there
static uint16_t calculate_checksum(unsigned char *data, int len)
{
    uint8_t *val = data;
    uint32_t sum = 0;
    for (int i = 0; i < (len + 1) / 2; i++) {
        uint16_t val16 = val[0] & 0xff;
        val16 = (uint16_t)(val16 << 8 | val[1]);
        val = val + 2;
        sum = val16 + sum;
    }
    while (sum & 0xffff0000) sum = (sum & 0xffff) + (sum >> 16);
    return (uint16_t)~sum;
}

// what ip_out does to the header of `line` for packet_id `id` (ip.c:102,106,107)
static void expect(const uint8_t *line, uint16_t id, uint8_t *out)
{
    memcpy(out, line, 64);
    out[24] = out[25] = 0;
    memcpy(out + 18, &id, 2);  // hdr->packet_id = count++ (x86: little-endian, no swap)
    const uint16_t ck = calculate_checksum(out + 14, 20);
    out[24] = (uint8_t)(ck >> 8);  // htons
    out[25] = (uint8_t)(ck & 0xff);
}

static void one(const uint8_t *line, uint16_t id)
{
    uint8_t want[64];
    expect(line, id, want);
    uint8_t *got = (uint8_t *)malloc(64);
    memcpy(got, line, 64);
    rxg_reset_set_id(got, id);
    CHECK(memcmp(got, want, 64) == 0);
    rxg_reset_set_id(got, id);  // again: nothing changes
    CHECK(memcmp(got, want, 64) == 0);
    free(got);
}

int main()
{
    // a reset as rxg_tx_reset_dev builds it (checksum fields as they happen to be)
    uint8_t base[64] = {0x02, 0x00, 0x0a, 0x00, 0x00, 0x01, 0x6a, 0x9c, 0xba, 0xa0, 0x96, 0x24, 0x08, 0x00,
                        0x45, 0x00, 0x00, 0x28, 0x34, 0x12, 0x00, 0x00, 0x7f, 0x06, 0xde, 0xad,
                        192, 168, 78, 2, 10, 0, 0, 1,
                        0x00, 0x50, 0x04, 0x00, 1, 2, 3, 4, 0, 0, 0, 0, 0x50, 0x04, 0xe0, 0x2e, 0xbe, 0xef, 0, 0};
    const uint16_t ids[] = {0, 1, 0x00FF, 0xFF00, 0xFFFF};
    for (uint16_t id : ids) one(base, id);
    {   // the last address word chosen so that the header's words sum to a multiple of 0xFFFF:
        // the folded sum is 0xFFFF and the checksum 0x0000
        for (uint16_t id : ids) {
            uint8_t l[64];
            memcpy(l, base, 64);
            l[24] = l[25] = l[32] = l[33] = 0;
            memcpy(l + 18, &id, 2);
            uint32_t s = 0;
            for (int i = 14; i < 34; i += 2) s += (uint32_t)(l[i] << 8 | l[i + 1]);
            const uint32_t w = (0xFFFFu - s % 0xFFFFu) % 0xFFFFu;
            l[32] = (uint8_t)(w >> 8);
            l[33] = (uint8_t)(w & 0xff);
            uint8_t want[64];
            expect(l, id, want);
            CHECK(want[24] == 0 && want[25] == 0);
            one(l, id);
        }
    }
    for (int i = 0; i < 100000; ++i) {
        uint8_t l[64];
        for (int j = 0; j < 64; j += 8) {
            const uint64_t r = rnd();
            memcpy(l + j, &r, 8);
        }
        if (i & 1) memset(l + 14, (i & 2) ? 0xFF : 0x00, 20);  // all-ones / all-zero headers
        one(l, (uint16_t)rnd());
    }
    rxg_reset_set_id(nullptr, 7);  // a NULL line is left alone
    if (fails) return 1;
    printf("txreset ok\n");
    return 0;
}
