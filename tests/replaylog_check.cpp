// CPU check of the replay's staleness rule (csrc/rxg_replaylog.h): the packet loop
// of rxg_rx_replay played over the real rxg::ReplayLog and rxg::WriteSet, with the host classifier
// and the selected launch both replaced by a lookup ("frame j at epoch e has this record") and a
// writer frame's handler by the WriteSet its write leaves.  Nothing of the library is linked.
//
//   replaylog_check <case file>   prints, for tests/test_replaylog_host.py to compare with the model
//                                 of tests/replay_sel_cases.py (Case.sim):
//                                   seen <per frame the epoch whose record its handler saw>
//                                   launch <burst> <the list, indices within the burst>   (each)
//                                   stats <marked> <host fix-ups> <device fix-ups> <launches>
//   replaylog_check direct        two cases that need no model: two tuples that share a filter_hash,
//                                 one written (the other's packet is not stale); a packet fixed at
//                                 write number s against writes numbered <= s and a later one
//
// The case file (little-endian, written by the test): u32 magic, n, nbursts, nepochs, nwriters,
// on_device; u16 len[n]; u8 head[n][54] (a frame's first 54 bytes, zero-filled past its length);
// u32 burst[nbursts][2] (first frame, one past the last); rxg_rec16 rec[nepochs][n]; per writer in
// frame order: u32 frame, all, pass2, nkeys, nlisten, u32 key[nkeys][3], i32 listen[nlisten].
// Every frame is held in a heap block of min(len, 54) bytes, so that under ASan a read past a
// short frame's end is an error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "rxg_replaylog.h"

using namespace rxg;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

static constexpr uint32_t kMagic = 0x31435052u;  // "RPC1"
static constexpr size_t kHead = 54;

template <class T> static std::vector<T> take(FILE *f, size_t count)
{
    std::vector<T> v(count);
    CHECK(count == 0 || std::fread(v.data(), sizeof(T), count, f) == count);
    return v;
}

static int run_case(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    CHECK(f);
    const std::vector<uint32_t> h = take<uint32_t>(f, 6);
    CHECK(h[0] == kMagic);
    const uint32_t n = h[1], nbursts = h[2], nepochs = h[3], nwriters = h[4];
    const bool on_device = h[5] != 0;
    const std::vector<uint16_t> len = take<uint16_t>(f, n);
    const std::vector<uint8_t> head = take<uint8_t>(f, (size_t)n * kHead);
    const std::vector<uint32_t> bursts = take<uint32_t>(f, (size_t)nbursts * 2);
    const std::vector<rxg_rec16> recs = take<rxg_rec16>(f, (size_t)nepochs * n);
    std::map<uint32_t, WriteSet> writers;
    for (uint32_t w = 0; w < nwriters; ++w) {
        const std::vector<uint32_t> wh = take<uint32_t>(f, 5);
        WriteSet &s = writers[wh[0]];
        s.all = wh[1] != 0;
        s.pass2 = wh[2] != 0;
        const std::vector<uint32_t> keys = take<uint32_t>(f, (size_t)wh[3] * 3);
        for (uint32_t k = 0; k < wh[3]; ++k) s.keys.push_back(TupleKey{keys[3 * k], keys[3 * k + 1], keys[3 * k + 2]});
        s.listen = take<int32_t>(f, wh[4]);
    }
    CHECK(std::fgetc(f) == EOF);
    std::fclose(f);
    CHECK(writers.size() == nwriters && nwriters + 1 == nepochs);

    std::vector<std::unique_ptr<uint8_t[]>> blocks(n);
    std::vector<void *> frames(n);
    for (uint32_t j = 0; j < n; ++j) {
        const size_t keep = std::min<size_t>(len[j], kHead);
        blocks[j].reset(new uint8_t[keep ? keep : 1]);
        std::memcpy(blocks[j].get(), &head[(size_t)j * kHead], keep);
        frames[j] = blocks[j].get();
    }

    // the context's part: the writes since the last absorb, those of this launch's replays so
    // far, and the log (kept across the bursts, as rxg_ctx keeps it)
    WriteSet touched, launch_writes;
    ReplayLog log;
    uint32_t e = 0;                      // the table's epoch: writers so far
    std::vector<uint32_t> seen(n, 0u);   // per frame the epoch of the record its handler saw
    std::vector<uint32_t> sel;
    for (uint32_t b = 0; b < nbursts; ++b) {
        const uint32_t lo = bursts[2 * b], m = bursts[2 * b + 1] - lo;
        CHECK(lo + m <= n);
        void *const *fr = frames.data() + lo;
        std::vector<uint32_t> at(m, 0u);  // the epoch of packet i's record: every burst was classified at 0
        log.begin(m, recs.data() + lo, RXG_REC16);
        if (b > 0 && !launch_writes.empty()) log.absorb(launch_writes);
        if (!touched.empty()) {
            launch_writes.add(touched);
            log.absorb(touched);
            touched.clear();
        }
        for (uint32_t i = 0; i < m; ++i) {
            if (log.stale(i, fr)) {
                const ReplayLog::Plan p = log.plan(i, fr, m, on_device, sel);
                if (p == ReplayLog::kLaunch) {
                    std::printf("launch %u", b);
                    for (uint32_t j : sel) {
                        std::printf(" %u", j);
                        log.fixed(j, recs[(size_t)e * n + lo + j]);
                        at[j] = e;
                    }
                    std::printf("\n");
                } else {
                    log.fixed(i, recs[(size_t)e * n + lo + i]);
                    at[i] = e;
                }
                log.done(p, sel.size());
            }
            CHECK(log.as_burst(i) == (at[i] == 0u));
            seen[lo + i] = at[i];
            auto w = writers.find(lo + i);
            if (w != writers.end()) {  // its handler wrote the table
                CHECK(log.record(i).verdict == RXG_V_DISPATCH);
                touched.add(w->second);
                ++e;
                launch_writes.add(touched);
                log.absorb(touched);
                touched.clear();
            }
        }
    }
    CHECK(e + 1 == nepochs);
    std::printf("seen");
    for (uint32_t j = 0; j < n; ++j) std::printf(" %u", seen[j]);
    std::printf("\nstats %llu %llu %llu %llu\n", (unsigned long long)log.stats[0], (unsigned long long)log.stats[1],
                (unsigned long long)log.stats[2], (unsigned long long)log.stats[3]);
    return 0;
}

// A 54-byte frame whose frame_key is k.
static void frame_of(const TupleKey &k, uint8_t *f)
{
    std::memset(f, 0, kHead);
    f[26] = (uint8_t)(k.src >> 24), f[27] = (uint8_t)(k.src >> 16), f[28] = (uint8_t)(k.src >> 8), f[29] = (uint8_t)k.src;
    f[30] = (uint8_t)k.dst, f[31] = (uint8_t)(k.dst >> 8), f[32] = (uint8_t)(k.dst >> 16), f[33] = (uint8_t)(k.dst >> 24);
    f[34] = (uint8_t)(k.ports >> 8), f[35] = (uint8_t)k.ports, f[36] = (uint8_t)(k.ports >> 24), f[37] = (uint8_t)(k.ports >> 16);
    CHECK(frame_key(f) == k);
}

static rxg_rec16 dispatch_rec(int32_t idx)
{
    rxg_rec16 r;
    std::memset(&r, 0, sizeof r);
    r.tcb_idx = idx;
    r.verdict = RXG_V_DISPATCH;
    r.flags = RXG_F_IP_OK | RXG_F_TCP_OK;
    return r;
}

static int run_direct()
{
    // filter aliasing: the first two of a run of client tuples that share a filter_hash
    std::map<uint32_t, TupleKey> by_hash;
    TupleKey ka{}, kb{};
    bool found = false;
    for (uint32_t t = 0; t < 400000u && !found; ++t) {
        const TupleKey k{(80u << 16) | (1024u + (t & 0x7FFFu)), 0x024EA8C0u, 0x0A010000u + (t >> 15)};
        auto ins = by_hash.emplace(filter_hash(k), k);
        if (!ins.second) {
            ka = ins.first->second;
            kb = k;
            found = true;
        }
    }
    CHECK(found && !(ka == kb) && filter_hash(ka) == filter_hash(kb));
    uint8_t fa[kHead], fb[kHead];
    frame_of(ka, fa);
    frame_of(kb, fb);
    void *frames[2] = {fa, fb};
    const rxg_rec16 burst[2] = {dispatch_rec(4), dispatch_rec(5)};
    {
        ReplayLog log;
        log.begin(2, burst, RXG_REC16);
        CHECK(!log.stale(0, frames) && !log.stale(1, frames));
        WriteSet w;
        w.keys.push_back(ka);
        log.absorb(w);
        CHECK(log.stale(0, frames));   // its tuple was written
        CHECK(!log.stale(1, frames));  // the filter's bit is set, the exact lookup says no
        std::vector<uint32_t> sel;
        CHECK(log.plan(0, frames, 2, false, sel) == ReplayLog::kHost && sel.empty());
        CHECK(log.plan(0, frames, 2, true, sel) == ReplayLog::kLaunch && sel == std::vector<uint32_t>{0u});
    }
    // later write wins
    {
        ReplayLog log;
        log.begin(2, burst, RXG_REC16);
        WriteSet wa, wb;
        wa.keys.push_back(ka);
        wb.keys.push_back(kb);
        log.absorb(wa);  // write 1
        CHECK(log.stale(0, frames) && log.as_burst(0));
        log.fixed(0, dispatch_rec(7));  // fixed at write 1
        CHECK(!log.stale(0, frames) && !log.as_burst(0) && log.record(0).tcb_idx == 7);
        log.absorb(wb);  // write 2: another tuple
        CHECK(!log.stale(0, frames) && log.stale(1, frames));
        log.absorb(wa);  // write 3: its tuple again
        CHECK(log.stale(0, frames));
        log.fixed(0, dispatch_rec(8));  // fixed at write 3: fresh against 1 .. 3
        CHECK(!log.stale(0, frames));
        CHECK(log.stale(1, frames));    // still only as fresh as the burst
        log.begin(2, burst, RXG_REC16);  // the next burst starts clean
        CHECK(!log.stale(0, frames) && !log.stale(1, frames) && log.as_burst(0));
    }
    std::printf("direct ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: replaylog_check <case file> | direct\n");
        return 2;
    }
    return std::strcmp(argv[1], "direct") == 0 ? run_direct() : run_case(argv[1]);
}
