// CPU unit test of the device-table write ordering (csrc/rxg_tablesync.h)
// against a recording device.  The port logs every operation with its stream, keeps a host
// copy of the three tables and applies patch lists and uploads to it in the order the device
// would (all writes run on the context's stream; a carried list runs at its carrying launch),
// and answers "is A ordered before B" from same-stream order plus record -> wait edges (vector
// clocks, the host's own waits included).  Asserted as the operations are issued:
//   1. every table write is ordered before every table-reading launch issued after it;
//   2. every table-reading launch is ordered before every table write issued after it;
//   3. a patch buffer is rewritten or freed only when the launch that last read it is known
//      complete to the host (a table buffer likewise, against every launch that touched it);
//   4. a carried list holds at most kLaunchPatchMax patches, no two for one word;
//   5. after each sync has reached the device, its tables equal the mirrors' arrays;
//   6. the event another stream or the server path waits for covers the carrying launch
//      (1. for a stream; for the server, every write complete to the host);
// and no operation ever names a destroyed stream.  Built and run by tests/test_tablesync.py
// (also under ASan/UBSan).
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "rxg_mirror.h"
#include "rxg_tablesync.h"

using namespace rxg;

#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_scenario, #cond); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

static const char *g_scenario = "";

using Clock = std::vector<int>;  // per model stream: how many of its operations precede
static void join(Clock &a, const Clock &b)
{
    if (a.size() < b.size()) a.resize(b.size(), 0);
    for (size_t i = 0; i < b.size(); ++i) a[i] = std::max(a[i], b[i]);
}

struct RecPort {
    using Stream = int;  // a handle: 0 none, 1 the context's stream
    using Event = int;   // 0 none
    struct Op {
        int ms, pos;  // model stream and 1-based position on it
        bool writes, reads;
        Clock before;  // what precedes it
    };
    struct Ev {
        bool recorded = false;
        Clock at;
    };
    struct PatchMem {
        uint32_t cap;
        int last_reader;  // op index, -1 none
    };

    std::vector<Op> ops;
    std::vector<Clock> vc;          // per model stream
    std::vector<int> issued;        // per model stream
    Clock host;                     // what the host knows complete
    std::map<int, int> handle;      // live stream handle -> model stream
    std::map<int, Ev> evs;
    int next_ev = 1;
    std::map<MirrorPatch *, PatchMem> pmem;
    int carried_launches = 0, patch_launches = 0, uploads = 0, host_waits = 0, allocs = 0;
    std::vector<int> log;  // patch_launch: 1, carrying burst: 2, plain burst: 3, upload: 4

    RecPort() { create_stream(1); }

    void create_stream(int h)
    {
        CHECK(h != 0 && !handle.count(h));
        handle[h] = (int)vc.size();
        vc.emplace_back();
        issued.push_back(0);
    }
    void destroy_stream(int h) { CHECK(handle.erase(h) == 1); }
    int model(int h) const
    {
        auto it = handle.find(h);
        CHECK(it != handle.end());  // a destroyed (or never created) stream is named
        return it->second;
    }

    bool ordered(const Op &a, const Clock &before) const
    {
        return (size_t)a.ms < before.size() && before[a.ms] >= a.pos;
    }
    bool complete(int op) const { return op < 0 || ordered(ops[op], host); }

    int issue(int h, bool writes, bool reads)
    {
        const int ms = model(h);
        join(vc[ms], host);  // submitted after whatever the host has waited for
        Op o{ms, ++issued[ms], writes, reads, vc[ms]};
        for (const Op &p : ops) {
            if (p.writes && reads) CHECK(ordered(p, o.before));  // 1: writes before later readers
            if (p.reads && writes) CHECK(ordered(p, o.before));  // 2: readers before later writes
            if (p.writes && writes) CHECK(ordered(p, o.before)); // writes apply in issue order
        }
        if (vc[ms].size() <= (size_t)ms) vc[ms].resize(ms + 1, 0);
        vc[ms][ms] = o.pos;
        ops.push_back(o);
        return (int)ops.size() - 1;
    }

    // ---- the Port
    Stream stream() const { return 1; }
    int event_create(Event *e, bool)
    {
        *e = next_ev++;
        evs[*e] = Ev{};
        return 0;
    }
    void event_destroy(Event e) { CHECK(evs.erase(e) == 1); }
    int record(Event e, Stream s)
    {
        CHECK(evs.count(e));
        const int ms = model(s);
        join(vc[ms], host);
        evs[e].recorded = true;
        evs[e].at = vc[ms];
        return 0;
    }
    int stream_wait(Stream s, Event e)
    {
        CHECK(evs.count(e) && evs[e].recorded);
        join(vc[model(s)], evs[e].at);
        return 0;
    }
    int host_wait(Event e)
    {
        CHECK(evs.count(e) && evs[e].recorded);
        join(host, evs[e].at);
        ++host_waits;
        return 0;
    }
    int sync()
    {
        join(host, vc[model(1)]);
        return 0;
    }
    int patch_alloc(MirrorPatch **p, uint32_t cap, bool dev)
    {
        CHECK(dev == large_bar);
        *p = (MirrorPatch *)std::malloc((size_t)cap * sizeof(MirrorPatch));
        pmem[*p] = PatchMem{cap, -1};
        ++allocs;
        return 0;
    }
    int patch_free(MirrorPatch *p, bool dev)
    {
        CHECK(dev == large_bar && pmem.count(p));
        CHECK(complete(pmem[p].last_reader));  // 3
        pmem.erase(p);
        std::free(p);
        return 0;
    }
    std::pair<MirrorPatch *const, PatchMem> &owner(const MirrorPatch *p, uint32_t n)
    {
        for (auto &m : pmem)
            if (p >= m.first && p + n <= m.first + m.second.cap) return m;
        const bool inside_a_patch_buffer = false;
        CHECK(inside_a_patch_buffer);
        std::abort();
    }
    void patch_write(MirrorPatch *dst, const MirrorPatch *src, uint32_t n, bool dev)
    {
        CHECK(dev == large_bar);
        CHECK(complete(owner(dst, n).second.last_reader));  // 3
        std::memcpy(dst, src, (size_t)n * sizeof(MirrorPatch));
    }
    void apply(const MirrorPatch *list, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i) {
            const MirrorPatch &q = list[i];
            if (q.target == kPatchBucket) {
                CHECK(((size_t)q.index + 1) * 16 <= t_buckets->bytes);
                std::memcpy((char *)t_buckets->p + (size_t)q.index * 16, q.v, 16);
            } else if (q.target == kPatchListen) {
                CHECK(((size_t)q.index + 1) * 4 <= t_listen->bytes);
                std::memcpy((char *)t_listen->p + (size_t)q.index * 4, q.v, 4);
            } else {
                CHECK(q.target == kPatchArp && ((size_t)q.index + 1) * 4 <= t_arp->bytes);
                std::memcpy((char *)t_arp->p + (size_t)q.index * 4, q.v, 4);
            }
        }
    }
    int patch_launch(const MirrorPatch *list, uint32_t n, const DevBuf &b, const DevBuf &l, const DevBuf &a)
    {
        CHECK(&b == t_buckets && &l == t_listen && &a == t_arp && n > 0);
        owner(list, n).second.last_reader = issue(1, true, false);
        apply(list, n);
        ++patch_launches;
        log.push_back(1);
        return 0;
    }
    int table_resize(DevBuf &b, size_t bytes)
    {
        if (b.bytes >= bytes && b.p) return 0;
        for (size_t i = 0; i < ops.size(); ++i) CHECK(complete((int)i));  // 3: the old buffer is idle
        std::free(b.p);
        b.p = std::calloc(1, bytes);
        b.bytes = bytes;
        return 0;
    }
    int table_upload(DevBuf &b, const void *src, size_t bytes)
    {
        CHECK(b.p && bytes <= b.bytes);
        issue(1, true, false);
        std::memcpy(b.p, src, bytes);
        ++uploads;
        log.push_back(4);
        return 0;
    }

    // ---- what the library does around TableSync: a table-reading launch on `s`, with the
    // carried list as its argument
    void launch_reader(Stream s, const MirrorPatch *list, uint32_t n)
    {
        if (list) {
            CHECK(s == 1 && large_bar && n <= kLaunchPatchMax);  // 4
            std::set<std::pair<uint32_t, uint32_t>> words;
            for (uint32_t i = 0; i < n; ++i) CHECK(words.insert({list[i].target, list[i].index}).second);
            owner(list, n).second.last_reader = issue(s, true, true);
            apply(list, n);
            ++carried_launches;
        } else {
            issue(s, false, true);
        }
        log.push_back(list ? 2 : 3);
    }
    bool writes_complete() const
    {
        for (size_t i = 0; i < ops.size(); ++i)
            if (ops[i].writes && !complete((int)i)) return false;
        return true;
    }

    bool large_bar = true;
    DevBuf *t_buckets = nullptr, *t_listen = nullptr, *t_arp = nullptr;
};

using TS = TableSync<RecPort>;

static rxg_tcb_tuple tuple(uint32_t i, uint8_t state = RXG_TCP_ESTABLISHED)
{
    rxg_tcb_tuple t{};
    t.dport = 1000 + (int32_t)(i % 50000);
    t.sport = 2000 + (int32_t)(i / 50000);
    t.ipv4_dst = 0x0A000001u;
    t.ipv4_src = 0x0B000000u + i;
    t.state = state;
    return t;
}

// A context in miniature: the mirrors, TableSync over the recording port, and the library's
// call sequences (launch_bursts, server_burst, rxg_tcb_sync, rxg_fini).
struct Rig {
    TS ts;
    TcbMirror mir;
    ArpMirror arp;
    bool arp_on = false;
    uint64_t srv_synced = 0;

    Rig(bool large_bar, bool lazy, uint32_t ntcb = 4000)
    {
        RecPort &p = ts.port;
        p.large_bar = large_bar;
        p.t_buckets = &ts.buckets;
        p.t_listen = &ts.listen;
        p.t_arp = &ts.d_arp;
        CHECK(ts.init(large_bar, lazy) == 0);
        CHECK(p.table_resize(ts.d_arp, 256) == 0);
        load(ntcb);
        burst(1);  // the first sync: whole tables
    }
    ~Rig()
    {
        CHECK(ts.port.sync() == 0 && ts.wait_readers(true) == 0);
        for (size_t i = 0; i < ts.port.ops.size(); ++i) CHECK(ts.port.complete((int)i));
        ts.destroy();
        CHECK(ts.port.pmem.empty() && ts.port.evs.empty());
        for (DevBuf *b : {&ts.buckets, &ts.listen, &ts.d_arp}) std::free(b->p);
    }
    void load(uint32_t n)
    {
        std::vector<rxg_tcb_tuple> t(n);
        for (uint32_t i = 0; i < n; ++i) t[i] = tuple(i);
        mir.load(t.data(), nullptr, (int32_t)n);
        ts.tcb_changed();
    }
    // n TCB writes, each changing one bucket word (and none growing the table)
    void tcb_writes(uint32_t n, uint32_t first = 0)
    {
        for (uint32_t i = first; i < first + n; ++i)
            mir.set_state((int32_t)i, mir.tcb[i].state == RXG_SYN_RECV ? RXG_TCP_ESTABLISHED : RXG_SYN_RECV);
        CHECK(!mir.need_rebuild && mir.patches.size() >= n);
        ts.tcb_changed();
    }
    void arp_load(uint32_t n)
    {
        arp_on = true;
        arp.clear();
        for (uint32_t i = 0; i < n; ++i) arp.add(0xC0A80000u + i);
        ts.arp_changed();
    }
    void arp_adds(uint32_t n)
    {
        const uint32_t base = 0xC0A80000u + (uint32_t)arp.ips.size();
        for (uint32_t i = 0; i < n; ++i) CHECK(arp.add(base + i));
        CHECK(!arp.need_rebuild && arp.patches.size() == n);
        ts.arp_changed();
    }
    int sync(bool carry) { return ts.sync(&mir, arp_on ? &arp : nullptr, carry); }
    // 5: the device tables equal the mirrors (nothing waits to be carried)
    void tables_equal()
    {
        uint32_t n;
        CHECK(ts.carried(&n) == nullptr && !ts.tcb_stale());
        CHECK(ts.buckets.bytes >= mir.slots.size() * sizeof(Slot) &&
              !std::memcmp(ts.buckets.p, mir.slots.data(), mir.slots.size() * sizeof(Slot)));
        CHECK(ts.listen.bytes >= mir.listen.size() * 4 && !std::memcmp(ts.listen.p, mir.listen.data(), mir.listen.size() * 4));
        if (arp_on && !arp.need_rebuild)
            CHECK(ts.d_arp.bytes >= arp.slots.size() * 4 && !std::memcmp(ts.d_arp.p, arp.slots.data(), arp.slots.size() * 4));
        const DevTable v = ts.view();
        CHECK(v.bucket_mask == mir.nb - 1 && v.ntcb == mir.ntcb() && v.min_null == mir.min_null);
        CHECK((const void *)v.buckets == ts.buckets.p && (const void *)v.listen == ts.listen.p);
    }
    // launch_bursts on stream st; returns whether the launch carried a list
    bool burst(int st, bool frames = true)
    {
        CHECK(ts.reader_allowed(st));
        CHECK(sync(st == 1 && frames) == 0);
        CHECK(ts.before(st) == 0);
        uint32_t n = 0;
        const MirrorPatch *list = ts.carried(&n);
        if (frames) {
            ts.port.launch_reader(st, list, n);
            if (n) CHECK(ts.carried_taken(st) == 0);
        } else {
            CHECK(list == nullptr);  // a launch of no frames is never made: nothing may wait for it
        }
        CHECK(ts.after(st) == 0);
        tables_equal();
        return list != nullptr;
    }
    // server_burst: the sync, then the host waits for the writes (6)
    void served()
    {
        CHECK(sync(false) == 0);
        CHECK(ts.host_wait_writes(&srv_synced) == 0);
        CHECK(ts.port.writes_complete());
        tables_equal();
    }
    int open_stream(int h)
    {
        ts.port.create_stream(h);
        if (ts.lazy_readers) ts.register_stream(h);
        return h;
    }
};

static void scenarios(bool bar, bool lazy)
{
    char name[96];
    auto scenario = [&](const char *s) {
        std::snprintf(name, sizeof name, "%s, %s, %s", s, bar ? "large BAR" : "no large BAR", lazy ? "lazy" : "per-launch");
        g_scenario = name;
    };

    scenario("a write between bursts on one caller stream");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.burst(2);
        r.tcb_writes(3);
        CHECK(!r.burst(2));
        r.burst(2);  // no write since: no second wait for the same event
        CHECK(r.ts.port.patch_launches == 1);
    }
    scenario("a write between bursts on two caller streams");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.open_stream(3);
        r.burst(2);
        r.tcb_writes(3);
        r.burst(3);
        r.tcb_writes(5);
        r.burst(2);
    }
    scenario("a write between bursts on the context's stream");
    {
        Rig r(bar, lazy);
        r.burst(1);
        r.tcb_writes(3);
        CHECK(r.burst(1) == bar);  // carried with a large BAR, its own launch without
        CHECK(r.ts.port.patch_launches == (bar ? 0 : 1));
        r.tcb_writes(3);
        CHECK(!r.burst(1, false));  // a burst of no frames carries nothing
    }
    scenario("two reader streams, then a write");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.open_stream(3);
        r.burst(2);
        r.burst(3);
        r.tcb_writes(2);
        CHECK(!r.burst(1));  // readers pending elsewhere: not carried
        r.burst(2);
        r.burst(3);
    }
    scenario("more reader streams than entries");
    {
        Rig r(bar, lazy);
        for (int h = 2; h < 2 + 20; ++h) r.burst(r.open_stream(h));
        CHECK(r.ts.readers.size() == TS::kMaxReaderStreams);
        r.tcb_writes(2);
        r.burst(1);
        for (int h = 2; h < 2 + 20; ++h) r.burst(h);
        r.tcb_writes(2);
        r.served();
    }
    scenario("a stream retired before the next write, its handle reused");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.burst(2);
        if (lazy) CHECK(r.ts.retire(2) == 0);  // (per-launch mode asks for no retire)
        r.ts.port.destroy_stream(2);
        r.tcb_writes(2);
        r.burst(1);
        r.open_stream(2);  // a new stream with the old handle: it has waited for nothing
        r.tcb_writes(2);
        r.burst(1);
        r.burst(2);
        r.tcb_writes(2);
        r.burst(1);
    }
    if (lazy) {
        scenario("an unregistered stream is refused in lazy mode");
        Rig r(bar, lazy);
        r.ts.port.create_stream(2);
        CHECK(!r.ts.reader_allowed(2) && r.ts.reader_allowed(1));
        r.ts.register_stream(2);
        CHECK(r.ts.reader_allowed(2));
        CHECK(r.ts.retire(2) == 0 && !r.ts.reader_allowed(2));
    }
    scenario("a carried list, then a burst on another stream");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.tcb_writes(4);
        CHECK(r.burst(1) == bar);
        r.burst(2);
        r.tcb_writes(4);
        r.burst(2);
    }
    scenario("a carried list, then the server's wait");
    {
        Rig r(bar, lazy);
        r.tcb_writes(4);
        CHECK(r.burst(1) == bar);
        r.served();
        const int waits = r.ts.port.host_waits;
        r.served();  // nothing written since: no second wait
        CHECK(r.ts.port.host_waits == waits);
    }
    for (uint32_t narp : {250u, 300u}) {
        scenario(narp == 250u ? "a carried TCB list and an ARP list that fits beside it"
                              : "a carried TCB list and an ARP list that overflows it");
        for (int then = 0; then < 2; ++then) {
            Rig r(bar, lazy);
            r.open_stream(2);
            r.arp_load(600);
            r.burst(1);
            r.tcb_writes(4);
            r.arp_adds(narp);
            const int launches = r.ts.port.patch_launches;
            CHECK(r.burst(1) == bar);
            if (bar) CHECK(r.ts.port.patch_launches == launches + (narp == 250u ? 0 : 1));
            if (then == 0) r.burst(2);
            else r.served();
        }
    }
    scenario("a second sync of one table inside a defer window");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.tcb_writes(8);
        CHECK(r.sync(true) == 0);
        r.tcb_writes(8, 4);  // words 4..7 again, with newer values, and four more
        const size_t mark = r.ts.port.log.size();
        CHECK(r.burst(1) == bar);
        if (bar) {  // the older list went out first, in its own launch; the newer one is carried
            CHECK(r.ts.port.log.size() == mark + 2 && r.ts.port.log[mark] == 1 && r.ts.port.log[mark + 1] == 2);
        }
        r.burst(2);
        // and a rebuild of a table the carried list touches
        r.tcb_writes(8);
        CHECK(r.sync(true) == 0);
        r.load(9000);
        r.burst(1);
        r.burst(2);
    }
    scenario("an abandoned carried list");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.tcb_writes(6);
        CHECK(r.sync(true) == 0);
        uint32_t n = 0;
        CHECK((r.ts.carried(&n) != nullptr) == bar);
        CHECK(r.ts.abandon() == 0);  // the launch failed or was never made
        r.tables_equal();
        r.burst(2);
        r.tcb_writes(6);
        CHECK(r.sync(true) == 0);
        r.served();  // make_current sends a list still waiting out itself
    }
    scenario("a list longer than every buffer, and every buffer in flight");
    {
        Rig r(bar, lazy);
        r.open_stream(2);
        r.tcb_writes(1500);  // over the first capacity (1024): reallocated
        r.burst(1);
        for (int i = 0; i < 6; ++i) {  // own launches, no host wait between them
            r.tcb_writes(300);
            r.burst(i == 3 ? 2 : 1);
        }
        CHECK(r.ts.port.host_waits >= 2);  // the ring wrapped: the host waited for the oldest
        r.tcb_writes(3500);  // and past the reallocated capacity
        r.burst(1);
    }
    scenario("a rebuild that outgrows the buffers while a reader is pending");
    {
        Rig r(bar, lazy, 100);
        r.open_stream(2);
        r.arp_load(8);
        r.burst(2);
        const size_t bytes = r.ts.buckets.bytes;
        r.load(20000);
        r.arp_load(4000);
        r.burst(1);
        CHECK(r.ts.buckets.bytes > bytes);
        r.burst(2);
    }
    if (!bar) {
        scenario("nothing is ever carried");
        Rig r(bar, lazy);
        for (int i = 0; i < 6; ++i) {
            r.tcb_writes(2);
            CHECK(!r.burst(1));
        }
        CHECK(r.ts.port.carried_launches == 0 && r.ts.port.patch_launches == 6);
    }
}

int main()
{
    for (int bar = 1; bar >= 0; --bar)
        for (int lazy = 0; lazy < 2; ++lazy) scenarios(bar != 0, lazy != 0);
    std::puts("tablesync ok");
    return 0;
}
