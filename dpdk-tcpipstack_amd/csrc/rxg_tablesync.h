// rxg_tablesync.h — the order of device-table writes against the kernels that read the tables
// (DESIGN.md §2.4), as one owner of that state over a Port, so its rules run in a CPU unit test
// (tests/tablesync_check.cpp) with a recording device instead of a GPU.  No HIP call here.
//
// The rules.  Table writes run on the context's stream: a patch list in its own launch, a
// whole table uploaded after a rebuild, or a short list carried by the burst about to be
// launched on that stream.  A table-reading launch on another stream waits for mirror_ev, the
// event after the last write (once per write, not per launch); the next write waits for every
// other stream that launched a reader since the last one (one event per stream: recorded after
// the stream's latest such launch, or in lazy mode on the stream at the write, which keeps a
// marker packet per launch off the caller's stream but needs the stream to exist then:
// registered streams only).  While a list waits to be carried, mirror_ev is stale: it is
// recorded again after the carrying launch when another stream or the server next needs it.
// Each table's writes are applied in issue order: a write to a table the carried list touches
// sends the carried list out first.
//
// Port (rxg_host.cpp HipTablePort: the real stream, events and buffers).  Every int is 0 or a
// negative errno; Stream and Event are opaque, copyable handles, Stream{} names no stream:
//   Stream stream()                       the context's stream (writes run on it)
//   int event_create(Event *e, bool reader)  an event (reader: one that orders a reader stream)
//   void event_destroy(Event e)
//   int record(Event e, Stream s)         record e after everything `s` has taken so far
//   int stream_wait(Stream s, Event e)    later work on `s` waits for e's last recording
//   int host_wait(Event e)                the host waits for e's last recording
//   int sync()                            the host waits for the context's stream
//   int patch_alloc(MirrorPatch **p, uint32_t cap, bool dev)   a list buffer: device memory
//   int patch_free(MirrorPatch *p, bool dev)                   the host writes (dev), or pinned
//   void patch_write(MirrorPatch *dst, const MirrorPatch *src, uint32_t n, bool dev)
//                                         copy a list in and publish it to the device (the
//                                         launch that last read dst[0..n) has completed)
//   int patch_launch(const MirrorPatch *list, uint32_t n, const DevBuf &buckets,
//                    const DevBuf &listen, const DevBuf &arp)
//                                         apply the list on the context's stream (whatever
//                                         else rides along, the pending counter corrections,
//                                         is the port's business)
//   int table_resize(DevBuf &b, size_t bytes)   at least `bytes`; the old buffer is idle
//   int table_upload(DevBuf &b, const void *src, size_t bytes)   on the context's stream
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rxg_mirror.h"

namespace rxg {

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// patch lists longer than this go through their own launch (every workgroup of a launch that
// carries a list stores all of it)
inline constexpr uint32_t kLaunchPatchMax = 256;

template <class Port>
struct TableSync {
    using Stream = typename Port::Stream;
    using Event = typename Port::Event;
    static constexpr int kPatchBufs = 4;
    static constexpr size_t kMaxReaderStreams = 16;

    Port port;

    // device tables and what travels with them at launch (view())
    DevBuf buckets, listen, d_arp;
    uint32_t bucket_mask = 0, arp_mask = 0;
    int32_t dev_ntcb = 0;
    int32_t dev_min_null = INT32_MAX;
    bool dirty = true;       // TCB mirror writes not on the device yet
    bool arp_dirty = false;  // ARP mirror writes likewise

    Event mirror_ev{};
    bool mirror_ev_set = false;
    bool mirror_ev_stale = false;  // a write on the stream after mirror_ev's last recording
    uint64_t table_writes = 0;     // device table writes so far
    struct Reader {
        Stream s;
        Event e;
        bool pending;     // `s` launched a table reader since the last write (not yet waited for)
        bool recorded;    // e was recorded after that launch (per-launch mode)
        uint64_t waited;  // table_writes when `s` last waited for mirror_ev (~0: never)
    };
    std::vector<Reader> readers;
    bool lazy_readers = false;       // RXG_CFG_STREAMS_OUTLIVE_WRITES
    std::vector<Stream> registered;  // that mode's caller streams

    // Patch ring: a list is read by its patch launch or by the burst that carries it, so a
    // buffer is reused only after that launch ran; each buffer has its event, and the host
    // waits only when all of them are in flight (a patch launch waits on the device for bursts
    // running on caller streams, which can be long).
    struct PatchBuf {
        MirrorPatch *h = nullptr;
        uint32_t cap = 0;
        Event ev{};
        bool set = false;
    } patch[kPatchBufs];
    int patch_next = 0;
    // With a large BAR the buffers are device memory the host writes, and a launch on the
    // stream can carry a list itself: defer_patch asks apply_patches for that (inside sync()),
    // ip_* is the list waiting for its launch.
    bool patch_dev = false;
    bool defer_patch = false;
    const MirrorPatch *ip_list = nullptr;
    uint32_t ip_n = 0;
    int ip_buf = -1;
    uint32_t ip_tables = 0;  // 1 << target of every patch in the carried list

    int init(bool large_bar, bool lazy)
    {
        patch_dev = large_bar;
        lazy_readers = lazy;
        int rc = port.event_create(&mirror_ev, false);
        for (auto &pb : patch)
            if (!rc) rc = port.event_create(&pb.ev, false);
        return rc;
    }

    // Everything but the tables themselves (the context frees its device buffers together).
    void destroy()
    {
        for (auto &pb : patch) {
            if (pb.h) (void)port.patch_free(pb.h, patch_dev);
            if (pb.ev != Event{}) port.event_destroy(pb.ev);
            pb = PatchBuf{};
        }
        for (auto &r : readers) port.event_destroy(r.e);
        readers.clear();
        if (mirror_ev != Event{}) port.event_destroy(mirror_ev);
        mirror_ev = Event{};
    }

    // ---- the mirrors
    void tcb_changed() { dirty = true; }
    void arp_changed() { arp_dirty = true; }
    bool tcb_stale() const { return dirty; }

    // Bring the device tables up to date with the mirrors given (either may be null): the
    // changed words (usual) or, after a load or past load 1/2, the whole table.  No host block
    // on the patch path.  `carry`: the caller is about to launch a burst with frames on the
    // context's stream, which can take a short list as an argument (carried()).
    int sync(TcbMirror *m, ArpMirror *a, bool carry)
    {
        defer_patch = carry && patch_dev && !readers_pending();
        int rc = 0;
        if (m && dirty) {
            if (m->need_rebuild) {
                m->rebuild();
                rc = upload(1u << kPatchBucket | 1u << kPatchListen, buckets, m->slots.data(),
                            m->slots.size() * sizeof(Slot), &listen, m->listen.data(),
                            m->listen.size() * sizeof(int32_t));
            } else {
                rc = apply_patches(*m);
            }
            if (!rc) {
                bucket_mask = m->nb - 1;
                dev_ntcb = m->ntcb();
                dev_min_null = m->min_null;
                dirty = false;
            }
        }
        if (!rc && a && arp_dirty) {
            if (a->need_rebuild) {
                a->rebuild();
                rc = upload(1u << kPatchArp, d_arp, a->slots.data(), a->slots.size() * 4, nullptr, nullptr, 0);
            } else {
                rc = apply_patches(*a);
            }
            if (!rc) {
                arp_mask = a->nb - 1;
                arp_dirty = false;
            }
        }
        defer_patch = false;
        return rc;
    }

    DevTable view() const
    {
        DevTable t{};
        t.buckets = (decltype(t.buckets))buckets.p;
        t.listen = (const int32_t *)listen.p;
        t.arp = (decltype(t.arp))d_arp.p;
        t.bucket_mask = bucket_mask;
        t.ntcb = dev_ntcb;
        t.min_null = dev_min_null;
        t.arp_mask = arp_mask;
        return t;
    }

    // ---- the carried list: the launch on the context's stream that follows sync(.., true)
    // takes it as an argument and says so, or the caller abandons it
    const MirrorPatch *carried(uint32_t *n) const
    {
        *n = ip_n;
        return ip_n ? ip_list : nullptr;
    }

    // the launch on `st` took the list: its buffer is free again once that launch has run
    int carried_taken(Stream st)
    {
        ip_n = 0;
        if (int rc = port.record(patch[ip_buf].ev, st)) return rc;
        patch[ip_buf].set = true;
        return 0;
    }

    // A carried list no burst took (a failure between the sync and the launch, or a later
    // write to one of its tables): as its own launch, so no write is lost or reordered.
    int abandon()
    {
        if (ip_n == 0) return 0;
        const uint32_t n = ip_n;
        ip_n = 0;
        return launch_list(ip_buf, n);
    }

    // ---- readers
    // Lazy mode records an event on the reader's stream at the next write, so the stream must
    // still exist then: only a registered stream is known to (retire() ends that).  Asked
    // before anything changes for a launch; before() and after() rely on it.
    bool reader_allowed(Stream st) const { return st == port.stream() || !lazy_readers || is_registered(st); }

    // A launch on `st` that reads the tables follows the last write ...
    int before(Stream st)
    {
        if (st == port.stream() || !mirror_ev_set) return 0;
        // a stream that already waited for the current mirror_ev needs no second wait (each
        // wait is a barrier packet between the caller's launches)
        for (auto &x : readers)
            if (x.s == st && x.waited == table_writes) return 0;
        if (int rc = make_current()) return rc;  // (a write a burst carried: recorded now)
        if (int rc = port.stream_wait(st, mirror_ev)) return rc;
        for (auto &x : readers)
            if (x.s == st) x.waited = table_writes;
        return 0;
    }

    // ... and the next write follows it.
    int after(Stream st)
    {
        if (st == port.stream()) return 0;
        Reader *r = nullptr;
        for (auto &x : readers)
            if (x.s == st) r = &x;
        if (!r) {
            for (auto &x : readers)
                if (!x.pending) { r = &x; break; }
            if (!r && readers.size() >= kMaxReaderStreams) {
                // more reader streams than entries: the next write's stream waits for them now
                if (int rc = wait_readers(false)) return rc;
                r = &readers[0];
            }
            if (!r) {
                Event e{};
                if (int rc = port.event_create(&e, true)) return rc;
                readers.push_back({st, e, false, false, ~0ull});
                r = &readers.back();
            }
            // before() found no entry for st, so it has just waited for the current mirror_ev
            r->waited = mirror_ev_set ? table_writes : ~0ull;
            r->s = st;
        }
        r->pending = true;
        if (lazy_readers) {
            r->recorded = false;  // recorded by the next write (wait_readers)
        } else {
            if (int rc = port.record(r->e, st)) return rc;
            r->recorded = true;
        }
        return 0;
    }

    void register_stream(Stream st)
    {
        if (st != port.stream() && !is_registered(st)) registered.push_back(st);
    }

    // The order the next table write needs against this stream's launches, taken now; the
    // entry then names no stream (a new stream may get the same handle).
    int retire(Stream st)
    {
        if (st == port.stream()) return 0;
        for (auto &r : readers)
            if (r.s == st) {
                if (r.pending && !r.recorded) {
                    if (int rc = port.record(r.e, st)) return rc;
                    r.recorded = true;
                }
                r.s = Stream{};
                r.waited = ~0ull;
            }
        registered.erase(std::remove(registered.begin(), registered.end(), st), registered.end());
        return 0;
    }

    // Kernels that read the tables on other streams are done: before a write the context's
    // stream waits for them; before table buffers are freed or the counters are read
    // (`host`), the host does.  Lazy mode records the event now, on the reader's stream (it
    // covers every launch the stream has taken so far, the table readers among them).
    int wait_readers(bool host)
    {
        for (auto &r : readers)
            if (r.pending) {
                if (!r.recorded)
                    if (int rc = port.record(r.e, r.s)) return rc;
                if (int rc = host ? port.host_wait(r.e) : port.stream_wait(port.stream(), r.e)) return rc;
                r.pending = r.recorded = false;
            }
        return 0;
    }

    // ---- mirror_ev
    // mirror_ev follows every write issued so far: recorded on the stream if a write since its
    // last recording has not been.
    int make_current()
    {
        if (ip_n) return abandon();  // (not between a sync and its burst)
        if (!mirror_ev_stale) return 0;
        if (int rc = port.record(mirror_ev, port.stream())) return rc;
        mirror_ev_stale = false;
        return 0;
    }

    // The host has seen every table write land: `synced` is the caller's count of the writes
    // it has waited for (the latency-mode server reads the tables with no stream order).
    int host_wait_writes(uint64_t *synced)
    {
        if (table_writes == *synced) return 0;
        if (int rc = make_current()) return rc;
        if (int rc = port.host_wait(mirror_ev)) return rc;
        *synced = table_writes;
        return 0;
    }

  private:
    bool is_registered(Stream st) const
    {
        return std::find(registered.begin(), registered.end(), st) != registered.end();
    }

    bool readers_pending() const
    {
        for (const auto &r : readers)
            if (r.pending) return true;
        return false;
    }

    // a write was issued on the stream: mirror_ev after it.  A list a burst is still to carry
    // is written after this recording, so the event stays stale (make_current).
    int wrote()
    {
        if (int rc = port.record(mirror_ev, port.stream())) return rc;
        mirror_ev_set = true;
        mirror_ev_stale = ip_n != 0;
        return 0;
    }

    // patch[bi]'s first n patches as their own launch on the stream
    int launch_list(int bi, uint32_t n)
    {
        PatchBuf &pb = patch[bi];
        if (int rc = wait_readers(false)) return rc;
        if (int rc = port.patch_launch(pb.h, n, buckets, listen, d_arp)) return rc;
        if (int rc = port.record(pb.ev, port.stream())) return rc;
        pb.set = true;
        return wrote();
    }

    // One or two whole tables after a rebuild (`tables`: their patch-target bits).
    int upload(uint32_t tables, DevBuf &b0, const void *s0, size_t n0, DevBuf *b1, const void *s1, size_t n1)
    {
        int rc;
        if (ip_n != 0 && (ip_tables & tables) != 0)
            if ((rc = abandon())) return rc;  // the carried list's older writes come first
        if (n0 > b0.bytes || (b1 && n1 > b1->bytes)) {
            // the old buffers must be idle before they are freed
            if ((rc = wait_readers(true))) return rc;
            if ((rc = port.sync())) return rc;
            if ((rc = port.table_resize(b0, n0))) return rc;
            if (b1 && (rc = port.table_resize(*b1, n1))) return rc;
        }
        if ((rc = wait_readers(false))) return rc;
        if ((rc = port.table_upload(b0, s0, n0))) return rc;
        if (b1 && (rc = port.table_upload(*b1, s1, n1))) return rc;
        // the next write changes the mirror's arrays in place: the copies must have consumed them
        if ((rc = port.sync())) return rc;
        ++table_writes;
        return wrote();
    }

    // A mirror's patches (at most one per device word): into the next patch buffer, then in
    // one launch on the stream -- or, in a defer window, left for the burst to carry.
    template <class M>
    int apply_patches(M &mirror)
    {
        const std::vector<MirrorPatch> &p = mirror.patches;
        if (p.empty()) return 0;
        const uint32_t n = (uint32_t)p.size();
        uint32_t tables = 0;
        for (const MirrorPatch &q : p) tables |= 1u << q.target;
        if (ip_n != 0 && (ip_tables & tables) != 0) {
            // the carried list's older writes to these tables come first
            if (int rc = abandon()) return rc;
        } else if (ip_n != 0 && defer_patch) {
            // a second table's patches (the ARP mirror's after the TCB mirror's) join the list
            // the burst carries, when it has room (the kernel applies each by its target).
            // Every workgroup of the carrying launch stores the whole list in parallel, so no
            // two of its patches may write one word: a mirror emits at most one patch per
            // word, and only a list for tables the carried one does not touch joins it.
            PatchBuf &cb = patch[ip_buf];
            if (ip_n + n <= kLaunchPatchMax && ip_n + n <= cb.cap) {
                port.patch_write(cb.h + ip_n, p.data(), n, patch_dev);
                mirror.patches_taken();
                ++table_writes;
                ip_n += n;
                ip_tables |= tables;
                return 0;
            }
        }
        const int bi = patch_next;
        PatchBuf &pb = patch[bi];
        patch_next = (bi + 1) % kPatchBufs;
        if (pb.set)
            if (int rc = port.host_wait(pb.ev)) return rc;  // the launch that read this buffer is done
        pb.set = false;
        if (n > pb.cap) {
            if (pb.h)
                if (int rc = port.patch_free(pb.h, patch_dev)) return rc;
            pb.h = nullptr;
            pb.cap = 0;
            const uint32_t cap = std::max<uint32_t>(n * 2u, 1024u);
            if (int rc = port.patch_alloc(&pb.h, cap, patch_dev)) return rc;
            pb.cap = cap;
        }
        port.patch_write(pb.h, p.data(), n, patch_dev);
        mirror.patches_taken();
        ++table_writes;
        if (defer_patch && ip_n == 0 && n <= kLaunchPatchMax) {
            ip_list = pb.h;
            ip_n = n;
            ip_buf = bi;
            ip_tables = tables;
            mirror_ev_set = true;
            mirror_ev_stale = true;  // the carrying launch is the write (make_current)
            return 0;
        }
        return launch_list(bi, n);
    }
};

}  // namespace rxg
