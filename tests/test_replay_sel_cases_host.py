"""No GPU: the edge sets of tests/replay_sel_cases.py cover what they claim.  Every claim of the
layout (what a record names, what each writer touches), of the expectation (the epoch model equals
test_gpu_replay.sequential_reference for every set of at most 1 500 frames), of the model (the
restated rule gives every frame's handler the sequential record; lists, stats, slices, flushes and
look-aheads per set) and of the sets is an assertion here.

Snapshot against epochs: behind a `reload` every TCP frame that finds a row finds it at another
index, so a replay that fixed nothing fails on each of them.  Two kinds of selected frame keep
their record through a reload: a client's packet to port 9999 and a flow frame cut to 34 bytes
(ports read as zero) are RST_NOPCB against every table here; they are selected and re-classified
all the same, and the stats assertion counts them."""
import numpy as np
import pytest

import pktgen
import replay_sel_cases as rc
import rxg
import test_gpu_replay as tgr


def rec_key(r):
    return (int(r["verdict"]), int(r["tcb_idx"]), int(r["state"]), int(r["flags"]) & (rxg.F_LISTEN | rxg.F_REF_NULLSLOT))


def launches_of(c, on_device):
    return c.sim(on_device).launches


# ------------------------------------------------------------------------------ the layout ---
def test_table_and_frames_name_themselves():
    assert rc.F == 257 and len(rc.ROWS) == 262 and rc.ROWS[3] is None and rc.ROWS[2] == rc.L80 and rc.ROWS[261] == rc.L8080
    assert np.gcd(rc.F, 64) == 1
    tuples = [r[:4] for r in rc.ROWS if r is not None]
    assert len(set(tuples)) == len(tuples)
    c = rc.get("sizes/1025/64")
    r = c.cls(0)
    i = np.arange(c.n)
    assert (r["tcb_idx"] == 4 + i % rc.F).all() and (r["verdict"] == rxg.V_DISPATCH).all() and (r["state"] == rc.ESTABLISHED).all()
    assert not r["ip_cksum"].any() and not r["tcp_cksum"].any()
    # the spare rows' tuples and the listeners' keys are no frame's
    keys = {rc.key_of_frame(f) for n in rc.ALL for f in rc.get(n).frames if len(f) >= 54}
    assert not keys & {rc.key_of_row(x) for x in (rc.ROWS[0], rc.ROWS[1], rc.L80, rc.L8080)}
    # pass-2 packets: no row names a client
    c = rc.get("rewrites/a")
    r = c.cls(0)
    for i, s in enumerate(c.specs):
        if s[0] in ("syn", "ack"):
            want = {80: 2, 8080: 261, 9999: -1}[s[1]]
            assert r["tcb_idx"][i] == want and bool(r["flags"][i] & rxg.F_LISTEN) == (want >= 0)
            assert r["verdict"][i] == (rxg.V_RST_NOPCB if want < 0 else rxg.V_DISPATCH if s[0] == "syn"
                                       else rxg.V_RST_LISTEN_NONSYN)
            # the NULL slot at 3 lies above the port-80 listener and below everything else
            assert bool(r["flags"][i] & rxg.F_REF_NULLSLOT) == (s[1] != 80)
    for k in ("arp", "udp", "l2"):
        assert len(rc.NON_TCP[k]) == 64


def test_writers_touch_what_they_claim():
    t = rc.Table(rc.ROWS)
    w = rc.apply_writer(t, "listener")
    assert w.listen == [8080] and w.keys == [rc.key_of_row(rc.L8080)] and not w.all and not w.pass2
    assert t.rows[261] is None and t.min_null() == 3
    w = rc.apply_writer(t, "listener")            # appended again: Ntcb grows, no NULL slot appears
    assert w.listen == [8080] and not w.all and not w.pass2 and t.rows[262] == rc.L8080
    w = rc.apply_writer(t, "minnull")
    assert w.pass2 and not w.all and not w.listen and w.keys == [rc.key_of_row(rc.ROWS[0])] and t.min_null() == 0
    w = rc.apply_writer(t, ("tuple", 5))
    k = rc.key_of_row(rc.flow_row(5))
    assert w.keys == [k, k] and not (w.all or w.pass2 or w.listen) and t.rows[9] == rc.flow_row(5, rc.SYN_RECV)
    w = rc.apply_writer(t, ("tuple", 5))
    assert t.rows[9] == rc.flow_row(5)
    w = rc.apply_writer(t, "reload")
    assert w.all and not (w.keys or w.listen or w.pass2) and t.need_rebuild
    assert t.rows == [rc.ROWS[1], rc.L80, None] + rc.ROWS[4:261] + [None, rc.L8080, None]
    # a write while the load is pending sets touched.pass2 (rxg_tcb_upsert: mir.need_rebuild)
    assert rc.apply_writer(t, ("tuple", 5)).pass2
    t.pushed()
    assert not rc.apply_writer(t, ("tuple", 5)).pass2
    # minnull after a reload: the spare row at 0 lies below the listener at 1 and the NULL slot at 2
    t = rc.Table(rc.ROWS)
    rc.apply_writer(t, "reload")
    t.pushed()
    assert rc.apply_writer(t, "minnull").pass2 and t.rows[0] is None


# ------------------------------------------------------------------------- the expectation ---
class _Frame(bytes):
    """A frame that knows its place in the burst (the reference's handler is called with it)."""


def _pin_cases():
    seen, out = set(), []
    for n in rc.ALL:
        c = rc.get(n)
        sig = (tuple(c.specs), tuple(sorted(c.writers.items())), c.checks)
        if c.n <= 1500 and sig not in seen:
            seen.add(sig)
            out.append(n)
    return out


@pytest.mark.parametrize("name", _pin_cases())
def test_epoch_model_equals_the_sequential_reference(name, monkeypatch):
    c = rc.get(name)

    class WriterModel:
        def __init__(self, rows):
            self.t = rc.Table(rows)
            self.rows = self.t.rows

        def handle(self, idx, state, f):
            if f.i in c.writers:
                rc.apply_writer(self.t, c.writers[f.i])
                self.rows = self.t.rows

    monkeypatch.setattr(tgr, "Model", WriterModel)
    frames = []
    for i, f in enumerate(c.frames):
        g = _Frame(f)
        g.i = i
        frames.append(g)
    glob = {}
    out, cnt, rows = tgr.sequential_reference(rc.ROWS, frames, verify=c.checks, globals_out=glob)
    exp, ecnt, erows = c.expect
    assert rows == erows and cnt.tolist() == ecnt.tolist() and len(exp) == c.n
    nopcb = cksum = 0
    for i, r in enumerate(exp):
        if c.checks_drop(i):
            cksum += 1
            assert out[i] == (rxg.V_DROP_NONTCP, -1, rxg.STATE_NONE)
        else:
            nopcb += r["verdict"] == rxg.V_RST_NOPCB
            assert out[i] == (int(r["verdict"]), int(r["tcb_idx"]), int(r["state"])), i
    assert glob == dict(tcpnopcb=nopcb, tcpchecksumerror=cksum)


def test_pinned_sets_are_most_sets():
    pinned = {n.split("/")[0] for n in _pin_cases()}
    assert pinned == {"sizes", "holes", "classes", "waves", "rewrites", "trunc", "checks"}
    # forms' single-burst cases are rewrites/a's frames and writers (pinned once); the multi-burst
    # ones, waves' longer lists and the 20 000-frame holes are over 1 500 frames
    assert all(rc.get(n).n > 1500 or rc.get(n).specs == rc.get("rewrites/a").specs for n in rc.NAMES["forms"])


# -------------------------------------------------------------------------------- the model ---
@pytest.mark.parametrize("name", rc.ALL)
def test_model_gives_every_handler_the_sequential_record(name):
    """The restated rule is sequentially equivalent on every set and context kind, the epoch
    slices equal the whole-burst classification, and the snapshot differs from the expectation."""
    c = rc.get(name)
    exp, _, _ = c.expect
    for e in range(len(c.epochs)):
        a = 0 if e == 0 else sorted(c.writers)[e - 1] + 1
        b = sorted(c.writers)[e] + 1 if e < len(c.writers) else c.n
        assert exp[a:b].tobytes() == c.cls(e)[a:b].tobytes()
    for on_device, _ in rc.contexts(c):
        s = c.sim(on_device)
        assert len(s.seen) == c.n
        for i in range(c.n):
            assert rec_key(c.cls(s.seen[i])[i]) == rec_key(exp[i]), (name, on_device, i)
        assert s.marked >= len(s.launches) and s.dev == sum(len(l) for _, l in s.launches)
        for b, l in s.launches:
            lo, hi = c.bursts[b]
            assert l == sorted(set(l)) and 0 <= l[0] and l[-1] < hi - lo
    snap = c.cls(0)
    if not c.writers:
        assert exp.tobytes() == snap.tobytes()
        return
    assert exp.tobytes() != snap.tobytes()
    first = min(c.writers)
    if c.writers[first] == "reload":
        later = np.arange(c.n) > first
        tcp = np.isin(exp["verdict"], rc.TCP_VERDICTS)
        hit = later & tcp & (exp["tcb_idx"] >= 0)
        assert hit.any() and (exp["tcb_idx"][hit] != snap["tcb_idx"][hit]).all()
        same = later & tcp & np.array([rec_key(a) == rec_key(b) for a, b in zip(exp, snap)])      # RST_NOPCB in both
        for i in np.flatnonzero(same):
            assert c.specs[i] in (("syn", 9999), ("ack", 9999), ("cut", 34)), (name, i)


def test_dealing_model_on_known_lists():
    assert rc.need_slots(True) == 4 and rc.need_slots(False) == 6 and rc.RS16 == 11
    assert [rc.blocks_of(n, 1024) for n in (1, 4, 5, 313)] == [1, 1, 2, 79] and rc.blocks_of(97, 2) == 2
    small = rc.slices_of([64] * (64 * 12))
    fl = rc.flushes(small, 3)                     # the occupancy grid: a slice per wave, one flush at its end
    assert all(w == [([i], True)] for i, w in enumerate(fl))
    fl = rc.flushes(rc.slices_of([64] * (64 * 48)), 1)
    assert [[(len(s), f) for s, f in w] for w in fl] == [[(8, False), (4, True)]] * 4
    fl = rc.flushes(rc.slices_of(([100] + [64] * 63) * 49), 1)
    assert [(len(s), f) for s, f in fl[0]] == [(6, False), (6, False), (1, True)]
    assert [(len(s), f) for s, f in fl[1]] == [(6, False), (6, True)]
    assert rc.kind_of(small, 12) == "past" and rc.kind_of(small, 0) == "full"


# --------------------------------------------------------------------------------- the sets ---
def test_sizes():
    assert rc.SIZES_M == [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
    for ln in (64, 100):
        for m in rc.SIZES_M:
            c = rc.get(f"sizes/{m}/{ln}")
            assert c.n == m + 1 and c.writers == {0: "reload"} and set(c.lens) == {ln}
            d, v = c.sim(False), c.sim(True)
            if m <= rc.K_HOST_MAX:
                assert d.stats == dict(marked=m, host_fixups=m, device_fixups=0, device_launches=0)
            else:
                assert d.stats == dict(marked=1, host_fixups=0, device_fixups=m, device_launches=1)
                assert d.launches == [(0, list(range(1, m + 1)))]
            assert v.stats == dict(marked=1, host_fixups=0, device_fixups=m, device_launches=1)
            assert v.launches == [(0, list(range(1, m + 1)))]
            sl = rc.slices_of(c.sel_lens(v.launches[0]))
            assert all(rc.is_small(s) == (ln == 64 and len(s) == 64) for s in sl)
    assert {m % 64 for m in rc.SIZES_M} >= {0, 1, 63}


def test_holes():
    want = {"every_second": (500, 52), "lane63": (312, 56), "lane0": (312, 56), "last_alone": (1, 1),
            "spread300": (300, 44), "reversed": (500, 52)}
    for h, (m, last) in want.items():
        c = rc.get(f"holes/{h}")
        assert c.n <= 20000
        for on_device in (False, True):
            s = c.sim(on_device)
            if m <= rc.K_HOST_MAX and not on_device:
                assert s.stats == dict(marked=1, host_fixups=m, device_fixups=0, device_launches=0)
                continue
            ((b, l),) = s.launches
            assert len(l) == m and (m - 1) % 64 + 1 == last
            assert all(c.specs[i][0] == "flow" for i in l) and all(c.specs[i][0] in rc.NON_TCP for i in range(1, c.n) if i not in set(l))
            if m > 1:      # not a range: a list read as sel[k] = first + k names frames that are not selected
                assert l != list(range(l[0], l[0] + m)) and any(c.specs[l[0] + k][0] != "flow" for k in range(m))
    assert {i % 64 for i in launches_of(rc.get("holes/lane63"), True)[0][1]} == {63}
    assert {i % 64 for i in launches_of(rc.get("holes/lane0"), True)[0][1]} == {0}
    assert launches_of(rc.get("holes/last_alone"), True) == [(0, [19999])]
    assert launches_of(rc.get("holes/every_second"), True)[0][1] == list(range(1, 1001, 2))
    assert max(launches_of(rc.get("holes/spread300"), True)[0][1]) > 19000
    assert rc.get("holes/reversed").order == "rev" and rc.get("holes/every_second").order == "fwd"
    # all three kinds of frame that are never selected lie between the selected ones
    assert {s[0] for s in rc.get("holes/every_second").specs} == {"flow", "arp", "udp", "l2"}


def size_class(ln):
    for k, (lo, hi) in enumerate(rc.CLASS_RANGES):
        if ln <= hi:
            return k
    raise ValueError(ln)


def test_classes():
    edges = rc.CLASS_EDGES
    assert edges == [64, 65, 128, 129, 256, 257, 512, 513, 576, 577, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 9000]
    assert [hi for _, hi in rc.CLASS_RANGES[:-1]] == edges[0:-1:2] and [lo for lo, _ in rc.CLASS_RANGES[1:]] == edges[1:-1:2]
    c = rc.get("classes/mixed")
    for on_device in (False, True):      # past kHostReclassifyMax: the default context launches it too
        ((b, l),) = c.sim(on_device).launches
        sl = rc.slices_of(c.sel_lens((b, l)))
        assert len(sl) == 5 and sorted(x for x in sl[0] if x > 64) == edges[1:] and edges[0] in sl[0]
        assert all(rc.is_small(s) for s in sl[1:])
    c = rc.get("classes/per_class")
    for on_device in (False, True):
        ((b, l),) = c.sim(on_device).launches
        sl = rc.slices_of(c.sel_lens((b, l)))
        assert len(sl) == 10
        for k, s in enumerate(sl):
            lo, hi = rc.CLASS_RANGES[k]
            assert len(s) == 64 and {size_class(x) for x in s} == {k} and set(s) == {lo, hi}
        assert sum(x == 9000 for s in sl for x in s) == 1
    c = rc.get("classes/ahead")
    assert rc.contexts(c) == [(True, 1)]
    ((b, l),) = c.sim(True).launches
    sl = rc.slices_of(c.sel_lens((b, l)))
    assert len(sl) == len(rc.AHEAD) == 12 and rc.blocks_of(len(sl), 1) == 1
    ev = rc.lookaheads(sl, 1)
    assert {e[2] for e in ev} == set(rc.AHEAD_KINDS)
    assert [(w, s) for w, s, k in ev if k == "big0"] == [(1, 1)] and [(w, s) for w, s, k in ev if k == "big63"] == [(2, 2)]
    assert [(w, s) for w, s, k in ev if k == "partial"] == [(3, 7)] and [s for _, s, k in ev if k == "past"] == [8, 9, 10]
    # on the occupancy grid every look-ahead is past the list: only a capped grid meets the others
    assert {e[2] for e in rc.lookaheads(sl, rc.blocks_of(len(sl), 1024))} == {"past"}


def test_waves():
    for mb in (1, 2):
        for s in rc.WAVE_SLICES:
            for last in ("whole", "one"):
                for body in ("small", "class"):
                    c = rc.get(f"waves/{mb}/{s}/{last}/{body}")
                    assert rc.contexts(c) == [(True, mb)]
                    ((b, l),) = c.sim(True).launches
                    sl = rc.slices_of(c.sel_lens((b, l)))
                    assert len(sl) == s and len(sl[-1]) == (64 if last == "whole" else 1)
                    if body == "small":
                        assert all(rc.is_small(x) == (len(x) == 64) for x in sl)
                    else:
                        assert all(sum(v == 100 for v in x) == 1 and not rc.is_small(x) for x in sl)
                        assert len({x.index(100) for x in sl if len(x) == 64}) >= min(s - 1, 17)
                    fl = rc.flushes(sl, rc.blocks_of(s, mb))
                    per_wave = [len(range(w, s, 4 * mb)) for w in range(4 * mb)]
                    assert [sum(len(r) for r, _ in w) for w in fl] == per_wave
                    if mb == 1 and s in (48, 49) and body == "small" and last == "whole":
                        # 12 or 13 slices a wave: one flush of 8 before the wave's end
                        assert sorted(set(per_wave)) == ([12] if s == 48 else [12, 13])
                        assert all([f for _, f in w] == [False, True] and len(w[0][0]) == 8 for w in fl)
    early = {}      # per grid and body: some wave flushes before its end
    for n in rc.NAMES["waves"]:
        c = rc.get(n)
        sl = rc.slices_of(c.sel_lens(c.sim(True).launches[0]))
        fl = rc.flushes(sl, rc.blocks_of(len(sl), c.max_blocks))
        key = (c.max_blocks, n.split("/")[-1])
        early[key] = early.get(key, False) or any(not final for w in fl for _, final in w)
    assert early == {(1, "small"): True, (1, "class"): True, (2, "small"): True, (2, "class"): True}
    # a flushed ring holding the list's last, one-frame slice behind a flush before the wave's end
    c = rc.get("waves/1/49/one/small")
    fl = rc.flushes(rc.slices_of(c.sel_lens(c.sim(True).launches[0])), 1)
    assert [(len(r), f) for r, f in fl[0]] == [(8, False), (5, True)] and fl[0][1][0][-1] == 48


def test_rewrites():
    a, b = rc.get("rewrites/a"), rc.get("rewrites/b")
    n = rc.REWRITES_N
    assert a.writers == {0: "reload", 100: "minnull", 101: "listener", n - 2: ("tuple", (n - 1) % rc.F)}
    assert sorted(b.writers) == [0, 700, 701, n - 2] and {str(v) for v in b.writers.values()} == {str(v) for v in
                                                                                            [("tuple", 2), "listener", "minnull", "reload"]}
    p2 = [i for i, s in enumerate(a.specs) if s[0] in ("syn", "ack")]
    assert {a.specs[i] for i in p2} == set(rc.PASS2) and len([i for i in p2 if i > 101]) > rc.K_HOST_MAX
    d, v = a.sim(False), a.sim(True)
    # the reload's launch fixes everything behind frame 0; minnull's re-selects every pass-2 packet
    # of it (the listener write of frame 101 lands in the same scan); the tuple write leaves one
    assert [len(l) for _, l in d.launches] == [n - 1, len([i for i in p2 if i > 101])]
    assert d.launches[0][1] == list(range(1, n)) and d.launches[1][1] == [i for i in p2 if i > 101]
    assert set(d.launches[1][1]) < set(d.launches[0][1])
    assert d.stats == dict(marked=3, host_fixups=1, device_fixups=n - 1 + len(d.launches[1][1]), device_launches=2)
    assert v.launches[:2] == d.launches and v.launches[2] == (0, [n - 1]) and v.stats["host_fixups"] == 0
    # b: the tuple's packets alone (two before the next writer), then the dport's pass-2 packets
    # alone, then every pass-2 packet: host fix-ups on the default context, launches on the other
    d, v = b.sim(False), b.sim(True)
    mine = [i for i in range(1, n) if i % rc.F == 2 and b.specs[i][0] == "flow"]
    assert mine == [2, 516, 773] and v.launches[0] == (0, mine)
    p2 = [i for i, s in enumerate(b.specs) if s[0] in ("syn", "ack") and i > 701]
    assert v.launches[1] == (0, p2) and v.launches[2] == (0, [n - 1]) and len(v.launches) == 3
    assert d.launches == [] and d.stats["host_fixups"] == d.stats["marked"] == len(mine) + len(p2) + 1
    # a listener write alone leaves only its dport's pass-2 packets stale: the scan made at frame 701,
    # before that frame's own write, would have been those
    t = rc.Case("probe", b.specs, {0: ("tuple", 2), 700: "listener"})
    assert t.sim(True).launches[1] == (0, [i for i, s in enumerate(b.specs) if s[0] in ("syn", "ack") and s[1] == 8080 and i > 700])
    # what each writer moves in the expectation
    exp = a.expect[0]
    assert exp["tcb_idx"][n - 1] == a.cls(0)["tcb_idx"][n - 1] - 1 and exp["state"][n - 1] == rc.SYN_RECV
    i80 = next(i for i in range(102, n) if a.specs[i] == ("ack", 80))
    assert exp["flags"][i80] & rxg.F_REF_NULLSLOT and not a.cls(1)[i80]["flags"] & rxg.F_REF_NULLSLOT
    i8080 = next(i for i in range(102, n) if a.specs[i] == ("syn", 8080))
    assert exp["verdict"][i8080] == rxg.V_RST_NOPCB and a.cls(2)[i8080]["verdict"] == rxg.V_DISPATCH


def test_trunc():
    assert rc.TRUNC_LENS == [34, 40, 53, 54] and rc.TRUNC_N < rc.K_HOST_MAX
    for ln in rc.TRUNC_LENS:
        for at, i in (("first", 1), ("middle", 60), ("last", 120)):
            c = rc.get(f"trunc/{ln}/{at}")
            r = c.cls(0)
            assert c.lens[i] == ln and c.form == "host" and r["verdict"][i] in rc.TCP_VERDICTS
            assert bool(r["flags"][i] & rxg.F_TRUNC) == (ln < 54) and not (np.delete(r["flags"], i) & rxg.F_TRUNC).any()
            assert r["verdict"][i] == (rxg.V_RST_NOPCB if ln == 34 else rxg.V_DISPATCH)
            d, v = c.sim(False), c.sim(True)
            assert v.launches == [(0, list(range(1, 121)))]
            if ln == 54:
                assert d.launches == [] and d.stats["host_fixups"] == 120
            else:      # the frames before it are host fix-ups, everything stale from it on one launch
                assert d.launches == [(0, list(range(i, 121)))]
                assert d.stats == dict(marked=i, host_fixups=i - 1, device_fixups=121 - i, device_launches=1)
    c = rc.get("trunc/no_write")
    assert sum(ln < 54 for ln in c.lens) == 3 and c.sim(False).stats == c.sim(True).stats == dict(
        marked=0, host_fixups=0, device_fixups=0, device_launches=0)


def test_forms_and_checks():
    a = rc.get("rewrites/a")
    for f in rc.FORMS:
        for k in rc.KINDS:
            c = rc.get(f"forms/{f}/{k}")
            assert c.form == f and c.kind == k and c.specs[:a.n] == a.specs and c.writers == a.writers
            if f in ("multi", "smulti"):
                assert c.bursts == [(0, 1200), (1200, 1500), (1500, 1565)] and max(c.writers) < 1200
                d, v = c.sim(False), c.sim(True)
                # bursts 1 and 2 re-selected whole through launch_writes.all: a launch and 65 host fix-ups
                assert v.launches[3:] == [(1, list(range(300))), (2, list(range(65)))]
                assert d.launches[2:] == [(1, list(range(300)))] and d.stats["host_fixups"] == 1 + 65
            else:
                assert c.bursts == [(0, 1200)] and c.sim(True).launches == a.sim(True).launches
    assert rc.get("forms/dev/16").order == "shuffle" and set(a.lens) == {64}
    for n in rc.NAMES["checks"]:
        c = rc.get(n)
        assert c.checks and len(c.known_sources) >= 100
        bad = [i for i in range(c.n) if c.checks_drop(i)]
        tcpn = [i for i in range(c.n) if c.cls(0)["verdict"][i] in rc.TCP_VERDICTS]
        assert len(bad) == (len(tcpn) - 1) // 7 and 0 not in bad
        assert all(pktgen.tcp_checksum_of(c.frames[i]) != 0 for i in bad)
        srcs = {int.from_bytes(c.frames[i][26:30], "big") for i in tcpn}
        assert 0 < len(srcs & set(c.known_sources)) < len(srcs)
    assert rc.get("checks/sizes257").specs == rc.get("sizes/257/64").specs
    assert rc.get("checks/every_second").specs == rc.get("holes/every_second").specs
    # mixed lengths under the verify: the only place where a fix record's TCP_OK depends on `len`
    m = rc.get("checks/mixed")
    assert m.specs == rc.get("classes/mixed").specs and sorted(set(m.lens)) == rc.CLASS_EDGES
    assert any(m.checks_drop(i) for i in range(m.n)) and not all(m.checks_drop(i) for i in range(1, 65) if m.lens[i] > 64)


def test_names():
    assert list(rc.NAMES) == ["sizes", "holes", "classes", "waves", "rewrites", "trunc", "forms", "checks"]
    assert len(rc.ALL) == len(set(rc.ALL)) == 26 + 6 + 3 + 32 + 2 + 13 + 15 + 3
    assert max(rc.get(n).n for n in rc.ALL) == 20000
