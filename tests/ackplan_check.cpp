// ackplan_check.cpp — rxg_ack_plan_host run stand-alone over dumped case sets, every array in a heap
// block of exactly its size (state has ntcb entries, order cap_seg, trains cap_trains, rxopts n,
// segs and acks cap, opts opt_cap), so that a sanitizer build sees any access past one.
// Usage: ackplan_check in.bin out.bin.  in.bin: a u64 job count, then per job 14 u64 {nord, ntr, n,
// ntcb, has_rxopts, tsval_now, ip_id0, opt_plain, opt_base, opt_cap, has_opts, cap, cap_seg,
// cap_trains} and the arrays order (nord u32), trains (ntr), train_count (4 u64), state (ntcb),
// rxopts (n, if given), the constant blocks (opt_base, if opts are given).  out.bin: per job segs
// (cap), acks (cap), opts (opt_cap, if given), count (4 u64); outputs are pre-filled with 0xA5.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rxg.h"

static std::vector<uint8_t> slurp(const char *path)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + got);
    fclose(f);
    return v;
}

template <typename T>
static T *block(const uint8_t *&p, uint64_t count)
{
    T *b = (T *)malloc(count ? count * sizeof(T) : 1);
    if (count) memcpy(b, p, count * sizeof(T));
    p += count * sizeof(T);
    return b;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const std::vector<uint8_t> in = slurp(argv[1]);
    if (in.size() < 8) return 2;
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    const uint8_t *p = in.data();
    uint64_t jobs;
    memcpy(&jobs, p, 8);
    p += 8;
    for (uint64_t j = 0; j < jobs; ++j) {
        uint64_t h[14];
        memcpy(h, p, sizeof h);
        p += sizeof h;
        const uint64_t nord = h[0], ntr = h[1], n = h[2], ntcb = h[3], cap = h[11], opt_base = h[8], opt_cap = h[9];
        uint32_t *order = block<uint32_t>(p, nord);
        rxg_flow_train *trains = block<rxg_flow_train>(p, ntr);
        uint64_t *tcount = block<uint64_t>(p, 4);
        rxg_ack_state *state = block<rxg_ack_state>(p, ntcb);
        rxg_rx_opt *rxopts = h[4] ? block<rxg_rx_opt>(p, n) : nullptr;
        rxg_tx_opt *opts = nullptr;
        if (h[10]) {
            opts = (rxg_tx_opt *)malloc(opt_cap ? opt_cap * sizeof(rxg_tx_opt) : 1);
            memset(opts, 0xA5, opt_cap * sizeof(rxg_tx_opt));
            memcpy(opts, p, opt_base * sizeof(rxg_tx_opt));
            p += opt_base * sizeof(rxg_tx_opt);
        }
        rxg_tx_seg *segs = (rxg_tx_seg *)malloc(cap ? cap * sizeof(rxg_tx_seg) : 1);
        rxg_ack *acks = (rxg_ack *)malloc(cap ? cap * sizeof(rxg_ack) : 1);
        memset(segs, 0xA5, cap * sizeof(rxg_tx_seg));
        memset(acks, 0xA5, cap * sizeof(rxg_ack));
        uint64_t count[4];
        memset(count, 0xA5, sizeof count);
        rxg_dev_ack_plan a;
        memset(&a, 0, sizeof a);
        a.order = nord ? order : nullptr;
        a.cap_seg = h[12];
        a.trains = ntr ? trains : nullptr;
        a.cap_trains = h[13];
        a.train_count = tcount;
        a.n = (uint32_t)n;
        a.ntcb = (uint32_t)ntcb;
        a.rxopts = rxopts;
        a.state = state;
        a.tsval_now = (uint32_t)h[5];
        a.ip_id0 = (uint16_t)h[6];
        a.opt_plain = (uint32_t)h[7];
        a.opt_base = (uint32_t)opt_base;
        a.opt_cap = (uint32_t)opt_cap;
        a.opts = opts;
        a.segs = segs;
        a.acks = acks;
        a.cap = cap;
        a.count = count;
        const int rc = rxg_ack_plan_host(&a);
        if (rc) {
            printf("job %llu: rc %d\n", (unsigned long long)j, rc);
            return 1;
        }
        fwrite(segs, sizeof(rxg_tx_seg), cap, out);
        fwrite(acks, sizeof(rxg_ack), cap, out);
        if (opts) fwrite(opts, sizeof(rxg_tx_opt), opt_cap, out);
        fwrite(count, 8, 4, out);
        free(order);
        free(trains);
        free(tcount);
        free(state);
        free(rxopts);
        free(opts);
        free(segs);
        free(acks);
    }
    if (p != in.data() + in.size()) return 3;
    fclose(out);
    printf("ackplan ok %llu\n", (unsigned long long)jobs);
    return 0;
}
