"""GPU parity of the flow lookup (csrc/rxg_rx_classify.h) on the deterministic sets of
lookup_cases.py: the home bucket fetched per lane (the all-small run), four lanes to a bucket
through the LDS transpose (the class path) or not at all (a wave of flow-cache hits); the overflow
walks over tuples and ARP addresses by scalar loads (launched) and by vector loads (the resident
server), on chosen lanes, across the table's end, for a whole wave at once; the all-zero tuple
against free slots; the per-lane flow cache against one-bit neighbours of what it holds.  Every
case compares all record bytes of every frame, and all counters, with the oracle; expected values
never come from another kernel.
"""
import functools

import numpy as np
import pytest

import lookup_cases as lc
import oracle
import pktgen
import rxg

pytestmark = pytest.mark.gpu

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]


@pytest.fixture(scope="module", params=[1, 3])
def capped_engine(request):
    """A context whose rx grid is 1 or 3 workgroups (rxg_config.max_blocks): 4 or 12 waves, so a
    wave walks many slices and its flow cache lives across them."""
    eng = rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20, max_blocks=request.param)
    eng.blocks = request.param
    yield eng
    eng.close()


class Case:
    """Frames packed once with the oracle's answer against a table's final rows."""

    def __init__(self, t, frames, rows=None):
        self.t, self.frames = t, frames
        self.arena, self.off, self.lens = pktgen.pack_arena(frames)
        self.tcb, self.live = pktgen.table_arrays(t.final_rows if rows is None else rows)
        self.exp, self.ecnt = oracle.rx_batch(self.arena, self.off, self.lens, self.tcb, self.live)
        for a in (self.arena, self.off, self.lens, self.exp, self.ecnt):
            a.setflags(write=False)

    def want(self, kind, lo=0, hi=None, exp=None):
        e = (self.exp if exp is None else exp)[lo:hi]
        return e if kind == rxg.REC48 else e["c"] if kind == rxg.REC16 else rxg.rec8_pack(e["c"])


TABLES = {t.name: t for t in lc.launched_tables() + [lc.cache_table()]}
SETS = [(t.name, lname, form) for t in lc.launched_tables() for lname in lc.layouts(t) for form in lc.FORMS]


@functools.lru_cache(maxsize=None)
def cases(tname, lname, form):
    t = TABLES[tname]
    return [Case(t, lc.burst_frames(b, form)) for b in lc.layouts(t)[lname]]


@functools.lru_cache(maxsize=None)
def stream_case(tname, nwaves, form):
    t = TABLES[tname]
    steps = None if tname == "cache_table" else lc.zero_steps(t)
    return Case(t, lc.burst_frames(lc.cache_stream(nwaves, steps), form, lc.stream_small_fn(nwaves)))


def apply_ops(eng, ops):
    for op in ops:
        if op[0] == "remove":
            eng.tcb_remove(op[1])
        else:
            eng.tcb_upsert(op[1], *op[2], identifier=op[1] % 65535 + 1)


def load(eng, t, nops=None):
    """The table as loaded, synchronised (the rebuild), then its writes as patches."""
    eng.tcb_load(*pktgen.table_arrays(t.rows))
    eng.tcb_sync()
    apply_ops(eng, t.ops[:nops])


def assert_records(got, want, c, what, first=0):
    if got.tobytes() == want.tobytes():
        return
    n = len(want)
    gb = np.ascontiguousarray(got).view(np.uint8).reshape(n, -1)
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(n, -1)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    i = int(bad[0])
    raise AssertionError(f"{what}: records differ at {len(bad)} of {n} frames, first frame {first + i} (slice "
                         f"{(first + i) // 64}, lane {(first + i) % 64}, {len(c.frames[first + i])} bytes); lanes of "
                         f"the first slices: {sorted({int(b) % 64 for b in bad[:64]})}: got {got[i]} exp {want[i]}")


def run_rx(eng, c, kind, what, exp=None):
    eng.counters_reset()
    got = eng.rx_arena(c.arena, c.off, c.lens, kind)
    cnt = eng.counters()
    assert_records(got, c.want(kind, exp=exp), c, what)
    assert np.array_equal(cnt, c.ecnt), (what, cnt, c.ecnt)


# ---------------------------------------------------------------------------- launched ---

@pytest.mark.parametrize("tname,lname,form", SETS, ids=["-".join(s) for s in SETS])
def test_launched_capped(capped_engine, tname, lname, form):
    """Every table x layout x size form, every record kind, on one and on three workgroups."""
    load(capped_engine, TABLES[tname])
    for b, c in enumerate(cases(tname, lname, form)):
        for kind in KINDS:
            run_rx(capped_engine, c, kind, f"{tname} {lname}[{b}] {form} REC{kind} x{capped_engine.blocks}")


FULL = [s for s in SETS if s[1] in ("lane_rotation", "lane_walkers")]


@pytest.mark.parametrize("tname,lname,form", FULL, ids=["-".join(s) for s in FULL])
def test_launched_full_grid(engine, tname, lname, form):
    """One slice per wave: every wave's first probe, no cache carried over."""
    load(engine, TABLES[tname])
    for c in cases(tname, lname, form):
        for kind in KINDS:
            run_rx(engine, c, kind, f"{tname} {lname} {form} REC{kind} full grid")


@pytest.mark.parametrize("tname", ["tiny_wrap", "cluster16", "cluster16_removed", "zero_live_full", "zero_absent_full"])
def test_deep_small_runs(capped_engine, tname):
    """All-small lane_walkers repeated to 16 slices per wave (64 per workgroup): the launch takes
    the two-deep run (small_step2; REC8 and REC16, REC48 is never two-deep)."""
    t = TABLES[tname]
    burst = lc.padded(lc.lane_walkers(t)[0], 64 * capped_engine.blocks)
    c = Case(t, lc.burst_frames(burst, "small"))
    assert len(c.frames) >= 4096 * capped_engine.blocks and int(c.lens.max()) <= 64
    load(capped_engine, t)
    for kind in (rxg.REC8, rxg.REC16):
        run_rx(capped_engine, c, kind, f"deep {tname} REC{kind} x{capped_engine.blocks}")


@pytest.mark.parametrize("form", lc.FORMS)
def test_cache_stream(capped_engine, form):
    """The per-wave step sequence with as many waves as the grid has: every wave meets every step
    in order (over 16 slices per wave: REC8 / REC16 all-small runs are two-deep, REC48 one-deep)."""
    nwaves = 4 * capped_engine.blocks
    c = stream_case("cache_table", nwaves, form)
    load(capped_engine, c.t)
    for kind in KINDS:
        run_rx(capped_engine, c, kind, f"cache_stream({nwaves}) {form} REC{kind}")


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("zform", lc.ZERO_FORMS, ids=lambda z: f"{'live' if z[0] else 'absent'}_{'full' if z[1] else 'free'}")
def test_zero_tuple_first_in_the_cache(capped_engine, zform, form):
    """The all-zero tuple as a wave's first TCP frame: the cache's initial key words are zero and
    must not answer; live or absent, in a bucket with free slots or behind a full one."""
    t = lc.zero_tuple(*zform)
    c = stream_case(t.name, 4 * capped_engine.blocks, form)
    load(capped_engine, t)
    for kind in KINDS:
        run_rx(capped_engine, c, kind, f"zero stream {t.name} {form} REC{kind}")


@pytest.mark.parametrize("form", lc.FORMS)
def test_table_writes_between_launches(capped_engine, form):
    """cluster16, a burst, the removals and re-inserts (the backward shift moves keys across the
    table's end), the same burst: no cache entry or bucket of the first launch survives."""
    a, b = lc.cluster16(), lc.cluster16_removed()
    burst = lc.lane_walkers(a)[0] + lc.every_query(b)
    frames = lc.burst_frames(burst, form)
    ca, cb = Case(a, frames), Case(b, frames)
    assert ca.exp.tobytes() != cb.exp.tobytes()
    load(capped_engine, a)
    for kind in KINDS:
        run_rx(capped_engine, ca, kind, f"before the writes {form} REC{kind}")
    apply_ops(capped_engine, b.ops[a.setup_ops:])
    for kind in KINDS:
        run_rx(capped_engine, cb, kind, f"after the writes {form} REC{kind}")


# ------------------------------------------------------------------------------ served ---

def serve(eng, kind, blocks, plan):
    """plan: list of ("burst", Case, lo, hi) / ("ops", table writes) / ("arp", addresses learned).  Counters are reset before the server
    starts; records and counters are read after it has stopped (nothing is queued on the
    context's stream beside the resident server).  Returns [(Case, lo, hi, records)], counters."""
    bufs, out = {}, []
    try:
        for step in plan:
            if step[0] == "burst" and id(step[1]) not in bufs:
                c = step[1]
                bufs[id(c)] = (eng.to_device(c.arena), eng.to_device(c.off), eng.to_device(c.lens))
        total = sum(s[3] - s[2] for s in plan if s[0] == "burst")
        d_out = eng.alloc(total * kind)
        eng.counters_reset()
        eng.sync()
        eng.server_start(kind, blocks=blocks, max_frames=1 << 14)
        try:
            at = 0
            for step in plan:
                if step[0] == "ops":
                    apply_ops(eng, step[1])
                    continue
                if step[0] == "arp":
                    for ip in step[1]:
                        eng.arp_learned(ip)
                    continue
                _, c, lo, hi = step
                da, do, dl = bufs[id(c)]
                eng.server_burst_dev(da.ptr, do.ptr + 4 * lo, dl.ptr + 2 * lo, hi - lo, d_out.ptr + at * kind, kind)
                out.append((c, lo, hi, at))
                at += hi - lo
        finally:
            eng.server_stop()
        recs = d_out.download(rxg.rec_dtype(kind), total)
        cnt = eng.counters()
        d_out.free()
        return [(c, lo, hi, recs[at:at + hi - lo]) for c, lo, hi, at in out], cnt
    finally:
        for ds in bufs.values():
            for d in ds:
                d.free()


def check_served(res, cnt, kind, what, exps=None):
    ecnt = np.zeros(oracle.NCOUNTERS, dtype=np.uint64)
    for k, (c, lo, hi, got) in enumerate(res):
        exp = c.exp if exps is None else exps[k]
        assert_records(got, c.want(kind, lo, hi, exp=exp), c, f"{what} burst {k} [{lo}, {hi})", lo)
        ecnt += oracle.rx_batch(c.arena, c.off[lo:hi], c.lens[lo:hi], c.tcb, c.live)[1]
    assert cnt.tolist() == ecnt.tolist(), (what, cnt, ecnt)


def slice_plan(c):
    """Bursts of 1, 2 and 3 slices (the server's shared-slice forms lead the classify), a partial
    slice, then the whole set."""
    n = len(c.frames)
    cuts = [(0, 64), (64, 192), (192, 384), (384, 384 + 37), (0, n)]
    return [("burst", c, lo, min(hi, n)) for lo, hi in cuts if lo < n]


SERVED = ["tiny_wrap", "cluster16", "zero_live_free", "zero_absent_free", "zero_live_full", "zero_absent_full"]


@pytest.mark.parametrize("blocks", [1, 8])
@pytest.mark.parametrize("kind", [rxg.REC8, rxg.REC16, rxg.REC48])
def test_served_tables(kind, blocks):
    """The resident server's walks (VWALK: per lane, vector loads) against the oracle, not against
    a launch: walkers on chosen lanes, every lane, across the end; the zero tuple; writes made
    between two served bursts."""
    eng = rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20)
    try:
        for tname in SERVED:   # (one server session per table: its three size forms one after another)
            t = TABLES[tname]
            load(eng, t)
            plan = []
            for form in lc.FORMS:
                frames = lc.burst_frames((lc.lane_walkers(t)[0] if t.walkers else []) + lc.every_query(t), form)
                if tname.startswith("zero"):
                    frames += stream_case(tname, 4, form).frames
                plan += slice_plan(Case(t, frames))
            res, cnt = serve(eng, kind, blocks, plan)
            check_served(res, cnt, kind, f"served {tname} REC{kind} blocks {blocks}")
        a, b = lc.cluster16(), lc.cluster16_removed()
        load(eng, a)
        frames = lc.burst_frames(lc.lane_walkers(a)[0] + lc.every_query(b), "alt")
        ca, cb = Case(a, frames), Case(b, frames)
        plan = slice_plan(ca) + [("ops", b.ops[a.setup_ops:])] + slice_plan(cb)
        res, cnt = serve(eng, kind, blocks, plan)
        check_served(res, cnt, kind, f"served writes between bursts REC{kind} blocks {blocks}")
    finally:
        eng.close()


@pytest.mark.parametrize("blocks", [1, 8])
@pytest.mark.parametrize("form", lc.FORMS)
def test_served_cache_stream(form, blocks):
    eng = rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20)
    try:
        c = stream_case("cache_table", 4, form)
        load(eng, c.t)
        for kind in (rxg.REC8, rxg.REC16):
            n = len(c.frames)
            plan = [("burst", c, 0, n), ("burst", c, 0, 64), ("burst", c, 256 * 3, 256 * 3 + 128), ("burst", c, n - 192, n)]
            res, cnt = serve(eng, kind, blocks, plan)
            check_served(res, cnt, kind, f"served cache_stream {form} REC{kind} blocks {blocks}")
    finally:
        eng.close()


# ------------------------------------------------------------------------- other paths ---

@functools.lru_cache(maxsize=None)
def walkers_case(form="alt"):
    t = lc.cluster16()
    return Case(t, lc.burst_frames(lc.lane_walkers(t)[0], form))


@pytest.mark.parametrize("by_ref", [False, True])
def test_fused_handoff(capped_engine, by_ref):
    """rxg_rx_burst_payload_dev, copied and by reference: the PAY kernels' classify."""
    from oracle import payload as opl
    c = walkers_case()
    load(capped_engine, c.t)
    for kind in KINDS:
        capped_engine.counters_reset()
        recs, pay, msgs, (arena, off, lens) = capped_engine.rx_burst_payload(c.frames, kind, by_reference=by_ref)
        cnt = capped_engine.counters()
        assert np.array_equal(off, c.off) and np.array_equal(lens, c.lens)
        assert_records(recs, c.want(kind), c, f"fused by_ref={by_ref} REC{kind}")
        assert np.array_equal(cnt, c.ecnt), (cnt, c.ecnt)
        e_msgs, _ = opl.slots(c.frames, c.exp["c"], c.off)
        for name in ("arena_off", "len", "flags"):
            assert np.array_equal(msgs[name], e_msgs[name]), name


def test_multi_burst(capped_engine):
    """rxg_rx_bursts_dev: the lane_walkers slices as four bursts of one pool in one launch (MULTI),
    cut inside slices so that a walker's lane differs from its lane in the single burst."""
    c = walkers_case()
    eng = capped_engine
    load(eng, c.t)
    n = len(c.frames)
    cuts = [0, 64 + 31, 64 * 5 + 1, 64 * 9, n]
    for kind in KINDS:
        da, do, dl, dout = eng.to_device(c.arena), eng.to_device(c.off), eng.to_device(c.lens), eng.alloc(n * kind)
        try:
            eng.counters_reset()
            eng.rx_bursts_dev(da.ptr, [(do.ptr + 4 * a, dl.ptr + 2 * a, b - a, dout.ptr + kind * a)
                                       for a, b in zip(cuts, cuts[1:])], kind)
            eng.sync()
            cnt = eng.counters()
            got = dout.download(rxg.rec_dtype(kind), n)
        finally:
            for d in (da, do, dl, dout):
                d.free()
        assert_records(got, c.want(kind), c, f"multi-burst REC{kind}")
        assert np.array_equal(cnt, c.ecnt)


def test_strided(capped_engine):
    """rxg_rx_bursts_strided_dev: the same frames two slots apart, no offset list."""
    c0 = walkers_case()
    eng = capped_engine
    load(eng, c0.t)
    n, stride, slot0 = len(c0.frames), 2, 3
    arena = np.full((slot0 + n * stride) * 64, 0xA5, dtype=np.uint8)
    for i, f in enumerate(c0.frames):
        arena[(slot0 + i * stride) * 64:(slot0 + i * stride) * 64 + len(f)] = np.frombuffer(f, dtype=np.uint8)
    cuts = [0, 64 * 7 + 5, n]
    for kind in KINDS:
        da, dl, dout = eng.to_device(arena), eng.to_device(c0.lens), eng.alloc(n * kind)
        try:
            eng.counters_reset()
            eng.rx_bursts_strided_dev(da.ptr, stride, [(slot0 + a * stride, dl.ptr + 2 * a, b - a, dout.ptr + kind * a)
                                                       for a, b in zip(cuts, cuts[1:])], kind)
            eng.sync()
            cnt = eng.counters()
            got = dout.download(rxg.rec_dtype(kind), n)
        finally:
            for d in (da, dl, dout):
                d.free()
        assert_records(got, c0.want(kind), c0, f"strided REC{kind}")
        assert np.array_equal(cnt, c0.ecnt)


# --------------------------------------------------------------------------------- ARP ---

def arp_expected(c, members):
    """The oracle's records with F_ARP_LEARN where a TCP segment's source is no member (ip.c:30-32)."""
    exp = c.exp.copy()
    for i, f in enumerate(c.frames):
        if exp["c"]["verdict"][i] <= rxg.V_RST_LISTEN_NONSYN and int.from_bytes(f[26:30], "big") not in members:
            exp["c"]["flags"][i] |= rxg.F_ARP_LEARN
    return exp


def arp_case(nb, zero, form):
    a = lc.arp_cluster(nb, zero)
    t = lc.Table(f"arp{nb}", lc.ARP_TABLE_ROWS, [], 1)
    burst = lc.arp_burst(a)[0]
    return a, Case(t, lc.burst_frames(burst + burst[:1], form))


@pytest.mark.parametrize("form", lc.FORMS)
@pytest.mark.parametrize("nb,zero", [(4, False), (4, True), (16, False), (16, True)])
def test_arp_walks_launched(capped_engine, nb, zero, form):
    """An address cluster across the end of the ARP mirror: walkers on lanes 0, 31, 32, 63, on
    every lane, on the even ones; 0.0.0.0 with and without the zero flag."""
    a, c = arp_case(nb, zero, form)
    eng = capped_engine
    try:
        load(eng, c.t)
        eng.arp_load(a["known"])
        exp = arp_expected(c, set(a["known"]))
        assert (exp["c"]["flags"] & rxg.F_ARP_LEARN).any() and not (exp["c"]["flags"] & rxg.F_ARP_LEARN).all()
        for kind in KINDS:
            run_rx(eng, c, kind, f"arp nb {nb} zero {zero} {form} REC{kind}", exp=exp)
        for ip in a["later"]:
            eng.arp_learned(ip)
        if a["later"]:
            exp2 = arp_expected(c, set(a["known"] + a["later"]))
            assert exp2.tobytes() != exp.tobytes()
            for kind in KINDS:
                run_rx(eng, c, kind, f"arp nb {nb} learned {form} REC{kind}", exp=exp2)
    finally:
        eng.arp_disable()


@pytest.mark.parametrize("form", lc.FORMS)
def test_arp_learned_between_two_cached_launches(capped_engine, form):
    """A stream of repeating tuples whose sources are unknown: every lane's cache replays the
    flag; the sources are learned between two launches and the flag must drop in the second."""
    eng = capped_engine
    nwaves = 4 * eng.blocks
    c = stream_case("cache_table", nwaves, form)
    srcs = sorted({int.from_bytes(f[26:30], "big") for f, v in zip(c.frames, c.exp["c"]["verdict"]) if v <= 2})
    known = srcs[::3] + [pktgen.ip4(10, 250, i, 1) for i in range(40)]
    try:
        load(eng, c.t)
        eng.arp_load(known)
        exp = arp_expected(c, set(known))
        for kind in KINDS:
            run_rx(eng, c, kind, f"arp cache_stream {form} REC{kind}", exp=exp)
        for ip in srcs[1::3]:
            eng.arp_learned(ip)
        exp2 = arp_expected(c, set(known) | set(srcs[1::3]))
        assert exp2.tobytes() != exp.tobytes() and (exp2["c"]["flags"] & rxg.F_ARP_LEARN).any()
        for kind in KINDS:
            run_rx(eng, c, kind, f"arp cache_stream learned {form} REC{kind}", exp=exp2)
    finally:
        eng.arp_disable()


@pytest.mark.parametrize("blocks", [1, 8])
@pytest.mark.parametrize("nb,zero", [(4, False), (4, True), (16, False), (16, True)])
def test_arp_walks_served(nb, zero, blocks):
    eng = rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20)
    try:
        plan, exps = [], []
        for form in lc.FORMS + ("alt",):   # (the addresses are learned before the last, the server resident)
            a, c = arp_case(nb, zero, form)
            if len(plan) == 0:
                load(eng, c.t)
                eng.arp_load(a["known"])
            last = len(exps) == 3 * len(slice_plan(c))
            if last:
                plan.append(("arp", a["later"]))
            plan += slice_plan(c)
            exps += [arp_expected(c, set(a["known"] + (a["later"] if last else [])))] * len(slice_plan(c))
        res, cnt = serve(eng, rxg.REC16, blocks, plan)
        check_served(res, cnt, rxg.REC16, f"served arp nb {nb} zero {zero} blocks {blocks}", exps=exps)
    finally:
        eng.arp_disable()
        eng.close()
