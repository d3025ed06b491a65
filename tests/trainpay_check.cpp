// trainpay_check — rxg_train_payload_host as a stand-alone program (tests/test_trainpay_host.py
// builds it with and without ASan/UBSan).  Reads the cases the test wrote, runs each with every
// frame in a heap block of exactly its length and the arena and the messages in exactly sized
// blocks (a read past a frame or a write past a cap is a heap overflow the sanitizer sees) and
// writes what came back for the test to compare against the model.
//
// in:  u32 ncases, then per case: u32 rec_kind, n, cap_seg, cap_trains, flags, 0; u64 arena_cap;
//      n * rec_kind record bytes; n times {u16 len, len bytes}; cap_seg u32 order; cap_trains
//      rxg_flow_train; u64 count[4]
// out: per case: i32 rc, u64 arena_used, arena_cap bytes, n messages, cap_trains train messages
//      (everything 0xA5 before the call)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rxg.h"

static void rd(FILE *f, void *p, size_t bytes)
{
    if (bytes && fread(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
}

template <typename T>
static T *block(size_t count)
{
    T *p = count ? (T *)malloc(count * sizeof(T)) : nullptr;
    if (p) memset(p, 0xA5, count * sizeof(T));
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    rd(in, &ncases, 4);
    for (uint32_t k = 0; k < ncases; ++k) {
        uint32_t h[6];
        uint64_t arena_cap = 0;
        rd(in, h, sizeof h);
        rd(in, &arena_cap, 8);
        const uint32_t rec_kind = h[0], n = h[1], cap_seg = h[2], cap_trains = h[3], flags = h[4];
        void *recs = n ? aligned_alloc(16, ((size_t)n * rec_kind + 15) / 16 * 16) : nullptr;
        rd(in, recs, (size_t)n * rec_kind);
        std::vector<uint8_t *> frames;
        std::vector<uint16_t> len;
        for (uint32_t i = 0; i < n; ++i) {
            uint16_t l = 0;
            rd(in, &l, 2);
            uint8_t *f = (uint8_t *)malloc(l ? l : 1);
            rd(in, f, l);
            frames.push_back(f);
            len.push_back(l);
        }
        uint32_t *order = block<uint32_t>(cap_seg);
        rxg_flow_train *trains = block<rxg_flow_train>(cap_trains);
        rd(in, order, (size_t)cap_seg * 4);
        rd(in, trains, (size_t)cap_trains * sizeof(rxg_flow_train));
        uint64_t count[4];
        rd(in, count, sizeof count);
        uint8_t *arena = block<uint8_t>((size_t)arena_cap);
        rxg_payload_msg *msgs = block<rxg_payload_msg>(n), *tmsgs = block<rxg_payload_msg>(cap_trains);
        uint64_t used = ~0ull;
        const int32_t rc = rxg_train_payload_host(recs, rec_kind, (void *const *)frames.data(), len.data(), n, order,
                                                  cap_seg, trains, cap_trains, count, flags, arena, arena_cap, msgs, tmsgs,
                                                  &used);
        fwrite(&rc, 4, 1, out);
        fwrite(&used, 8, 1, out);
        if (arena) fwrite(arena, 1, (size_t)arena_cap, out);
        if (msgs) fwrite(msgs, sizeof *msgs, n, out);
        if (tmsgs) fwrite(tmsgs, sizeof *tmsgs, cap_trains, out);
        free(recs);
        for (uint8_t *f : frames) free(f);
        free(order);
        free(trains);
        free(arena);
        free(msgs);
        free(tmsgs);
    }
    fclose(in);
    fclose(out);
    puts("trainpay ok");
    return 0;
}
