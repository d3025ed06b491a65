// flowtrain_check — rxg_flow_trains_host as a stand-alone program (tests/test_flowtrain_host.py
// builds it with and without ASan/UBSan).  Reads the cases the test wrote, runs each with its
// outputs in exactly sized heap blocks (a write past a cap is a heap overflow the sanitizer sees)
// and writes what came back for the test to compare against the model.
//
// in:  u32 ncases, then per case: u32 rec_kind, n, ntcb, flags, has_cur, cap_seg, cap_trains;
//      n * rec_kind record bytes; for 8- and 16-byte records n times {u16 len, len bytes};
//      has_cur: ntcb u32
// out: per case: i32 rc, u64 count[4], cap_seg u32, cap_trains rxg_flow_train
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

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t ncases = 0;
    rd(in, &ncases, 4);
    for (uint32_t k = 0; k < ncases; ++k) {
        uint32_t h[7];
        rd(in, h, sizeof h);
        const uint32_t rec_kind = h[0], n = h[1], ntcb = h[2], flags = h[3], has_cur = h[4], cap_seg = h[5],
                       cap_trains = h[6];
        // exactly sized blocks, recs 16-byte aligned as a burst's are
        void *recs = n ? aligned_alloc(16, ((size_t)n * rec_kind + 15) / 16 * 16) : nullptr;
        rd(in, recs, (size_t)n * rec_kind);
        std::vector<uint8_t *> frames;
        std::vector<uint16_t> len;
        if (rec_kind != RXG_REC48) {
            for (uint32_t i = 0; i < n; ++i) {
                uint16_t l = 0;
                rd(in, &l, 2);
                uint8_t *f = (uint8_t *)malloc(l ? l : 1);
                rd(in, f, l);
                frames.push_back(f);
                len.push_back(l);
            }
        }
        uint32_t *cur = has_cur ? (uint32_t *)malloc((size_t)ntcb * 4) : nullptr;
        if (has_cur) rd(in, cur, (size_t)ntcb * 4);
        uint32_t *order = cap_seg ? (uint32_t *)malloc((size_t)cap_seg * 4) : nullptr;
        rxg_flow_train *trains = cap_trains ? (rxg_flow_train *)malloc((size_t)cap_trains * sizeof(rxg_flow_train)) : nullptr;
        if (order) memset(order, 0xA5, (size_t)cap_seg * 4);
        if (trains) memset(trains, 0xA5, (size_t)cap_trains * sizeof(rxg_flow_train));
        uint64_t count[4] = {~0ull, ~0ull, ~0ull, ~0ull};
        const int32_t rc = rxg_flow_trains_host(recs, rec_kind, frames.empty() ? nullptr : (void *const *)frames.data(),
                                                len.empty() ? nullptr : len.data(), n, ntcb, flags, cur, order, cap_seg,
                                                trains, cap_trains, count);
        fwrite(&rc, 4, 1, out);
        fwrite(count, 8, 4, out);
        if (order) fwrite(order, 4, cap_seg, out);
        if (trains) fwrite(trains, sizeof(rxg_flow_train), cap_trains, out);
        free(recs);
        for (uint8_t *f : frames) free(f);
        free(cur);
        free(order);
        free(trains);
    }
    fclose(in);
    fclose(out);
    puts("flowtrain ok");
    return 0;
}
