// lookup_check.cpp — where the host mirror (csrc/rxg_mirror.h) puts what the device flow
// lookup (csrc/rxg_rx_classify.h) reads: the probe path of given tuples and ARP addresses
// through the tables of tests/lookup_cases.py.
//
// Usage: lookup_check FILE.  FILE holds unsigned decimal words, one section after another:
//   T n      then n lines  dport sport ipv4_dst ipv4_src state live   (tcbs[] for load)
//   W m      then m lines  0 idx                                      (remove)
//                     or   1 idx dport sport ipv4_dst ipv4_src state  (upsert)
//   Q q      then q lines  ports dst_raw src_host                     (tuple queries)
//   A n      then n addresses (host order; 0 is the zero flag)        (ARP mirror, loaded)
//   L n      then n addresses learned after the rebuild (patched in)
//   R q      then q addresses                                         (ARP queries)
// It loads and rebuilds the TCB mirror, answers the tuple queries (phase 0), applies the writes
// and answers them again (phase 1, only with m > 0); the ARP mirror likewise before (phase 0)
// and after the learned addresses (phase 1, only with L > 0).  One line per answer:
//   T phase i nb hash home found probed crossed idx state listen
//   A phase i nb hash home found probed crossed hit
// found: the bucket the key sits in or -1; probed: buckets read; crossed: the walk went from
// bucket nb - 1 to bucket 0.  The walk here is restated from the table's description
// (rxg_common.h) and must agree with TcbMirror::find / ArpMirror::lookup, or the program says
// FAIL and exits 1.  Last line: "ok moves M rescans R".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rxg_mirror.h"

using namespace rxg;

static bool rd(FILE *f, uint64_t &v) { return std::fscanf(f, "%" SCNu64, &v) == 1; }

static uint64_t need(FILE *f)
{
    uint64_t v = 0;
    if (!rd(f, v)) {
        std::printf("FAIL short input\n");
        std::exit(1);
    }
    return v;
}

static rxg_tcb_tuple tuple_in(FILE *f, int32_t idx)
{
    rxg_tcb_tuple t{};
    t.dport = (int32_t)(int64_t)need(f);  // (ports outside 0..65535 travel as two's complement)
    t.sport = (int32_t)(int64_t)need(f);
    t.ipv4_dst = (uint32_t)need(f);
    t.ipv4_src = (uint32_t)need(f);
    t.state = (uint8_t)need(f);
    t.identifier = (uint16_t)(idx % 65535 + 1);
    return t;
}

struct Key {
    uint32_t ports, dst, src;
};

static int tuple_answers(const TcbMirror &m, const std::vector<Key> &q, int phase)
{
    const uint32_t mask = m.nb - 1;
    for (size_t i = 0; i < q.size(); ++i) {
        const uint32_t h = tuple_hash(q[i].ports, q[i].dst, q[i].src);
        uint32_t b = h & mask, probed = 0;
        int found = -1, crossed = 0;
        uint32_t val = kEmpty;
        for (;;) {
            ++probed;
            bool free_slot = false;
            for (int s = 0; s < kSlotsPerBucket; ++s) {
                const Slot &e = m.slots[(size_t)b * kSlotsPerBucket + s];
                if (e.val == kEmpty)
                    free_slot = true;
                else if (e.ports == q[i].ports && e.dst == q[i].dst && e.src == q[i].src && found < 0) {
                    found = (int)b;
                    val = e.val;
                }
            }
            if (found >= 0 || free_slot || probed == m.nb) break;
            if (b == mask) crossed = 1;
            b = (b + 1) & mask;
        }
        uint8_t st = 0;
        bool lh = false;
        const int32_t idx = m.find(q[i].ports, q[i].dst, q[i].src, q[i].ports >> 16, &st, &lh);
        if (found >= 0 ? (lh || idx != (int32_t)(val & kIdxMask) || st != (uint8_t)(val >> kStateShift))
                       : (idx != m.listen[q[i].ports >> 16] || lh != (idx >= 0))) {
            std::printf("FAIL tuple query %zu phase %d: the walk and find() disagree\n", i, phase);
            return 1;
        }
        std::printf("T %d %zu %u %u %u %d %u %d %d %u %d\n", phase, i, m.nb, h, h & mask, found, probed, crossed, idx,
                    (unsigned)st, (int)lh);
    }
    return 0;
}

static int arp_answers(const ArpMirror &a, const std::vector<uint32_t> &q, int phase)
{
    const uint32_t mask = a.nb - 1;
    for (size_t i = 0; i < q.size(); ++i) {
        const uint32_t ip = q[i], h = arp_hash(ip);
        uint32_t b = h & mask, probed = 0;
        int found = -1, crossed = 0;
        if (ip != 0u) {  // (0.0.0.0 is a flag: no bucket is read for it)
            for (;;) {
                ++probed;
                bool free_key = false;
                for (int k = 0; k < kArpKeysPerBucket; ++k) {
                    const uint32_t x = a.slots[(size_t)b * kArpKeysPerBucket + k];
                    if (x == ip) found = (int)b;
                    free_key |= x == 0u;
                }
                if (found >= 0 || free_key || probed == a.nb) break;
                if (b == mask) crossed = 1;
                b = (b + 1) & mask;
            }
        }
        const bool hit = ArpMirror::lookup(a.slots.data(), a.nb, a.has_zero, ip);
        if (ip != 0u && hit != (found >= 0)) {
            std::printf("FAIL arp query %zu phase %d: the walk and lookup() disagree\n", i, phase);
            return 1;
        }
        std::printf("A %d %zu %u %u %u %d %u %d %d\n", phase, i, a.nb, h, h & mask, found, probed, crossed, (int)hit);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<rxg_tcb_tuple> tcb;
    std::vector<uint8_t> live;
    struct Write {
        bool upsert;
        int32_t idx;
        rxg_tcb_tuple t;
    };
    std::vector<Write> writes;
    std::vector<Key> q;
    std::vector<uint32_t> arp, learned, aq;
    for (int c; (c = std::fgetc(f)) != EOF;) {
        if (c == ' ' || c == '\n') continue;
        const uint64_t n = need(f);
        for (uint64_t i = 0; i < n; ++i) {
            if (c == 'T') {
                tcb.push_back(tuple_in(f, (int32_t)i));
                live.push_back((uint8_t)need(f));
            } else if (c == 'W') {
                Write w{need(f) != 0, (int32_t)need(f), rxg_tcb_tuple{}};
                if (w.upsert) w.t = tuple_in(f, w.idx);
                writes.push_back(w);
            } else if (c == 'Q') {
                const uint32_t p = (uint32_t)need(f), d = (uint32_t)need(f), s = (uint32_t)need(f);
                q.push_back(Key{p, d, s});
            } else if (c == 'A') {
                arp.push_back((uint32_t)need(f));
            } else if (c == 'L') {
                learned.push_back((uint32_t)need(f));
            } else if (c == 'R') {
                aq.push_back((uint32_t)need(f));
            } else {
                std::printf("FAIL section '%c'\n", c);
                return 1;
            }
        }
    }
    std::fclose(f);

    TcbMirror m;
    m.load(tcb.data(), live.data(), (int32_t)tcb.size());
    m.rebuild();
    if (tuple_answers(m, q, 0)) return 1;
    if (!writes.empty()) {
        for (const Write &w : writes) {
            if (w.upsert)
                m.upsert(w.idx, w.t);
            else
                m.remove(w.idx);
        }
        if (m.need_rebuild) {
            std::printf("FAIL the writes ask for a rebuild\n");
            return 1;
        }
        if (tuple_answers(m, q, 1)) return 1;
    }

    ArpMirror a;
    for (uint32_t ip : arp) a.add(ip);
    a.rebuild();
    if (arp_answers(a, aq, 0)) return 1;
    if (!learned.empty()) {
        for (uint32_t ip : learned) a.add(ip);
        if (a.need_rebuild) {
            std::printf("FAIL the learned addresses ask for a rebuild\n");
            return 1;
        }
        if (arp_answers(a, aq, 1)) return 1;
    }
    std::printf("ok moves %" PRIu64 " rescans %" PRIu64 "\n", m.moves, m.rescans);
    return 0;
}
