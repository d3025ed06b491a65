// CPU check of what a replay hands out (csrc/rxg_attached.h): a script of the calls
// the C entry points of rxg_replay.cpp and the packet loop of rxg_rx_replay make, played over the
// real rxg::ReplayAttached, rxg::RcvWindow, rxg::ReplayLog, rxg::WriteSet and rxg::TcbMirror.
// Nothing of the library is linked but rxg_txresetid.cpp (rxg_reset_set_id, stand-alone host code).
//
//   attached_check <script>   one command a line; every answer is printed as one line, for
//                             tests/test_attached_host.py to compare with the model of
//                             tests/attached_cases.py (Model.run)
//
// The context's part
//   tcb <idx> <dport> <sport> <dst> <src>   mirror upsert (ESTABLISHED)
//   tcbrm <idx>                             mirror remove
//   touch all | touch key <ports> <dst> <src> | touch clear      rxg_ctx::touched
//   recs <n> {<verdict> <tcb_idx>}*n        the records of the burst the next `begin` replays
// The attachments (each array a heap block of exactly its length, kept until the program ends)
//   resets <n> {<pkt> <ip_id>}*n            64-byte frames built with that id   -> (nothing)
//   opts <n>                                                                   -> (nothing)
//   sums <m> {<tcb> <first> <last>}*m                                          -> sums ok | sums bad <k>
//   trains <nseg> {<pkt>}*nseg <nt> {<tcb> <first> <nseg>}*nt                   -> trains ok | trains bad <k> <expected first>
//   acks <n> <stride> {<tcb> <seq> <ack>}*n                                     -> acks ok | acks bad <a>
// The replay
//   begin <n> | beginfail <n>               begin_replay (+ ReplayLog::begin | + end_replay(false))
//   absorb <all> <nkeys> {<ports> <dst> <src>}*nkeys     a batch of writes: wrote + ReplayLog::absorb
//   fix <j> <verdict> <tcb_idx>             packet j re-classified: refixed + ReplayLog::fixed
//   at <i>
//   end <ran_to_end>
// The takes
//   reset <ip_id>      -> reset -1 | reset <slot> <the 64 bytes, hex>
//   opt                -> opt -1 | opt <record index>
//   sum                -> sum -1 | sum <entry> <pkt>
//   train              -> train -1 | train <train> <pos>
//   ack <tcb> <snd_nxt> <rcv_ack>   -> ack -1 | ack <entry>
// The receive window
//   rcvset <idx> <cur> <pairs>   -> rcvsize <entries>
//   rcvforget <idx> | rcvclear
//   pay <idx> <seq> <length> <msg flags> <msg len>   -> pay 0 | pay 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "rxg_attached.h"

using namespace rxg;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                \
        }                                                                \
    } while (0)

// A heap block of exactly n T's, zeroed, alive until the program ends (NULL for n == 0).
template <class T> static T *block(uint64_t n)
{
    static std::vector<std::unique_ptr<T[]>> keep;
    if (!n) return nullptr;
    keep.emplace_back(new T[n]());
    return keep.back().get();
}

static rxg_rec16 rec_of(uint32_t verdict, int32_t tcb)
{
    rxg_rec16 r;
    std::memset(&r, 0, sizeof r);
    r.verdict = (uint8_t)verdict;
    r.tcb_idx = tcb;
    r.flags = RXG_F_IP_OK | RXG_F_TCP_OK;
    return r;
}

// The reset frame the script's model builds for (slot k, ip_id): a pattern, the id, its checksum.
static void reset_frame(uint8_t *f, uint64_t k, uint16_t ip_id)
{
    for (int b = 0; b < 64; ++b) f[b] = (uint8_t)(17 * k + 3 * b + 1);
    rxg_reset_set_id(f, ip_id);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: attached_check <script>\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    CHECK(in.good());

    TcbMirror mir;
    WriteSet touched;
    ReplayLog log;
    ReplayAttached att;
    RcvWindow rcv;
    std::vector<rxg_rec16> recs;
    // the attached arrays' bases, to print an answer as an index
    uint8_t *rst = nullptr, *ak_frames = nullptr;
    const rxg_rx_opt *opts = nullptr;
    const rxg_flow_sum *sums = nullptr;
    const rxg_flow_train *trains = nullptr;
    uint32_t ak_stride = 0;

    std::string line, cmd;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        if (!(s >> cmd)) continue;
        if (cmd == "tcb") {
            int32_t idx;
            rxg_tcb_tuple t;
            std::memset(&t, 0, sizeof t);
            s >> idx >> t.dport >> t.sport >> t.ipv4_dst >> t.ipv4_src;
            t.state = RXG_TCP_ESTABLISHED;
            mir.upsert(idx, t);
        } else if (cmd == "tcbrm") {
            int32_t idx;
            s >> idx;
            mir.remove(idx);
        } else if (cmd == "touch") {
            std::string what;
            s >> what;
            if (what == "all") touched.all = true;
            else if (what == "clear") touched.clear();
            else {
                TupleKey k;
                s >> k.ports >> k.dst >> k.src;
                touched.keys.push_back(k);
            }
        } else if (cmd == "recs") {
            uint32_t n;
            s >> n;
            recs.clear();
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t v;
                int32_t t;
                s >> v >> t;
                recs.push_back(rec_of(v, t));
            }
        } else if (cmd == "resets") {
            uint64_t n;
            s >> n;
            rst = block<uint8_t>(64 * n);
            uint32_t *idx = block<uint32_t>(n);
            for (uint64_t k = 0; k < n; ++k) {
                uint32_t id;
                s >> idx[k] >> id;
                reset_frame(rst + 64 * k, k, (uint16_t)id);
            }
            att.attach_resets(rst, idx, n);
        } else if (cmd == "opts") {
            uint32_t n;
            s >> n;
            opts = block<rxg_rx_opt>(n);
            att.attach_opts(opts, n);
        } else if (cmd == "sums") {
            uint64_t m, bad = 0;
            s >> m;
            rxg_flow_sum *a = block<rxg_flow_sum>(m);
            for (uint64_t k = 0; k < m; ++k) s >> a[k].tcb_idx >> a[k].first_idx >> a[k].last_idx;
            if (att.attach_flow_sums(a, m, &bad)) {
                sums = a;
                std::printf("sums ok\n");
            } else {
                std::printf("sums bad %llu\n", (unsigned long long)bad);
            }
        } else if (cmd == "trains") {
            uint64_t nseg, nt, bad = 0, first = 0;
            s >> nseg;
            uint32_t *order = block<uint32_t>(nseg);
            for (uint64_t k = 0; k < nseg; ++k) s >> order[k];
            s >> nt;
            rxg_flow_train *t = block<rxg_flow_train>(nt);
            for (uint64_t k = 0; k < nt; ++k) s >> t[k].tcb_idx >> t[k].first >> t[k].nseg;
            if (att.attach_flow_trains(order, nseg, t, nt, &bad, &first)) {
                trains = t;
                std::printf("trains ok\n");
            } else {
                std::printf("trains bad %llu %llu\n", (unsigned long long)bad, (unsigned long long)first);
            }
        } else if (cmd == "acks") {
            uint64_t n, bad = 0;
            uint32_t stride;
            s >> n >> stride;
            rxg_ack *a = block<rxg_ack>(n);
            for (uint64_t k = 0; k < n; ++k) s >> a[k].tcb_idx >> a[k].seq >> a[k].ack;
            uint8_t *fr = block<uint8_t>(n * stride);
            if (att.attach_acks(a, fr, stride, n, &bad)) {
                ak_frames = fr;
                ak_stride = stride;
                std::printf("acks ok\n");
            } else {
                std::printf("acks bad %llu\n", (unsigned long long)bad);
            }
        } else if (cmd == "begin" || cmd == "beginfail") {
            uint32_t n;
            s >> n;
            att.begin_replay(n);
            if (cmd == "beginfail") {  // an argument check of rxg_rx_replay refused
                att.end_replay(false);
            } else {
                CHECK(n == recs.size());
                log.begin(n, recs.data(), RXG_REC16);
            }
        } else if (cmd == "absorb") {
            WriteSet w;
            uint32_t all, nk;
            s >> all >> nk;
            w.all = all != 0;
            for (uint32_t k = 0; k < nk; ++k) {
                TupleKey key;
                s >> key.ports >> key.dst >> key.src;
                w.keys.push_back(key);
            }
            att.wrote(w);
            log.absorb(w);
        } else if (cmd == "fix") {
            uint32_t j, v;
            int32_t t;
            s >> j >> v >> t;
            CHECK(j < log.size());
            const rxg_rec16 r = rec_of(v, t);
            att.refixed(log.record(j), r);
            log.fixed(j, r);
        } else if (cmd == "at") {
            uint32_t i;
            s >> i;
            att.at(i);
            CHECK(att.position() == (int64_t)i);
        } else if (cmd == "end") {
            int ran;
            s >> ran;
            att.end_replay(ran != 0);
            CHECK(att.position() == -1);
        } else if (cmd == "reset") {
            uint32_t id;
            s >> id;
            const uint8_t *f = att.take_reset((uint16_t)id);
            if (!f) {
                std::printf("reset -1\n");
            } else {
                CHECK((f - rst) % 64 == 0);
                std::printf("reset %lld ", (long long)((f - rst) / 64));
                for (int b = 0; b < 64; ++b) std::printf("%02x", f[b]);
                std::printf("\n");
            }
        } else if (cmd == "opt") {
            const rxg_rx_opt *o = att.opt_current();
            std::printf("opt %lld\n", o ? (long long)(o - opts) : -1ll);
        } else if (cmd == "sum") {
            uint32_t pkt = 0xFFFFFFFFu;
            const rxg_flow_sum *e = att.flow_sum_current(log, &pkt);
            if (e) std::printf("sum %lld %u\n", (long long)(e - sums), pkt);
            else std::printf("sum -1\n");
        } else if (cmd == "train") {
            uint32_t p = 0xFFFFFFFFu;
            const rxg_flow_train *t = att.flow_train_current(log, &p);
            if (t) std::printf("train %lld %u\n", (long long)(t - trains), p);
            else std::printf("train -1\n");
        } else if (cmd == "ack") {
            int32_t t;
            uint32_t seq, ack;
            s >> t >> seq >> ack;
            const uint8_t *f = att.ack_take(t, seq, ack, mir, touched);
            if (f) {
                CHECK((f - ak_frames) % ak_stride == 0);
                std::printf("ack %lld\n", (long long)((f - ak_frames) / ak_stride));
            } else {
                std::printf("ack -1\n");
            }
        } else if (cmd == "rcvset") {
            int32_t idx;
            uint32_t cur, pairs;
            s >> idx >> cur >> pairs;
            rcv.set(idx, cur, pairs != 0);
            std::printf("rcvsize %zu\n", rcv.size());
        } else if (cmd == "rcvforget") {
            int32_t idx;
            s >> idx;
            rcv.forget(idx);
        } else if (cmd == "rcvclear") {
            rcv.clear();
        } else if (cmd == "pay") {
            int32_t idx;
            uint32_t seq, length;
            rxg_payload_msg m;
            std::memset(&m, 0, sizeof m);
            s >> idx >> seq >> length >> m.flags >> m.len;
            std::printf("pay %d\n", rcv.take(idx, seq, length, m) ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown command: %s\n", line.c_str());
            return 2;
        }
        CHECK(!s.fail());
    }
    return 0;
}
