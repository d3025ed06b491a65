"""No GPU: the edge sets of tests/multiburst_cases.py cover what they claim.  Every claim of the
layout (what a record names, the descriptor tails, the guards, the REC8 alignment, the strided
pool) and of the sets (pairs, empties, counts, ring, runs, order) is an assertion here against the
generated sets and the module's model of the dealing: rx_args' slice numbering, the grid, the DEEP
rule, the waves' slices, the record ring's flushes and the look-aheads of the all-small runs.  The
model's claims are made for grids of one and two workgroups."""
import numpy as np
import pytest

import multiburst_cases as mc
import pktgen
import rxg

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
CAPPED = [1, 2]


def sl_of(c, launch):
    return mc.slices_of(launch, c.lens_of)


# ------------------------------------------------------------------------------ the layout ---
def test_table_and_spare_frame():
    assert len(mc.TCB) == mc.SPARE_ROW + 1 and mc.LIVE.all()
    tuples = {(int(r["ipv4_src"]), int(r["sport"])) for r in mc.TCB}
    assert len(tuples) == len(mc.TCB)                          # a tuple of its own per (burst, lane)
    assert mc.NB_TABLE >= max(mc.COUNT_KS) and max(mc.get(n).k for n in mc.ALL) <= mc.NB_TABLE
    import oracle
    pool = np.frombuffer(mc.SPARE, np.uint8)
    exp, _ = oracle.rx_batch(pool, np.zeros(1, np.uint32), np.array([64], np.uint16), mc.TCB, mc.LIVE)
    assert exp["c"]["tcb_idx"][0] == mc.SPARE_ROW and exp["c"]["verdict"][0] == rxg.V_DISPATCH
    assert exp["c"]["ip_cksum"][0] == 0 and exp["c"]["tcp_cksum"][0] == 0


@pytest.mark.parametrize("name", mc.ALL)
def test_records_name_burst_lane_and_slice(name):
    """The oracle's record of burst j's frame i: row j * 64 + i % 64, datalen (i // 64) % 11 for a
    small frame, valid checksums, dispatched; no record names the spare row."""
    c = mc.get(name)
    exp, cnt = c.oracle
    assert len(exp) == sum(c.ns) and int(cnt[0]) == sum(c.ns)
    pos = 0
    for j in range(c.k):
        n, r = c.ns[j], exp["c"][pos:pos + c.ns[j]]
        lens, i = np.array(c.lens[j], dtype=np.int64), np.arange(n)
        assert (r["tcb_idx"] == j * 64 + i % 64).all() and (r["verdict"] == rxg.V_DISPATCH).all()
        assert not r["ip_cksum"].any() and not r["tcp_cksum"].any()
        assert (r["datalen"] == lens - 54).all()
        assert (lens[lens <= 64] == 54 + (i[lens <= 64] // 64) % 11).all()
        assert ((lens >= 54) & ((lens <= 128) | (lens == 1500))).all()
        pos += n
    assert sum(ln == 1500 for b in c.lens for ln in b) <= 1
    # neighbours differ in REC8: the same lane of the next burst, the next lane, the next slice
    # (of the small frames; a frame over 64 bytes gives up the slice for its size)
    r8 = rxg.rec8_pack(exp["c"][np.concatenate([np.array(b, dtype=np.int64) for b in c.lens] + [np.zeros(0, np.int64)]) <= 64])
    assert len({(int(a), int(b)) for a, b in zip(r8["w0"], r8["w1"])}) == len(r8)


@pytest.mark.parametrize("name", mc.ALL)
def test_descriptors_pools_and_guards(name):
    c = mc.get(name)
    pool, offs = c.packed
    off_all, len_all, start = c.desc
    # end to end with no gap, in mem_order; TAIL entries of (slot 0, 64 bytes) behind
    pos = 0
    for j in c.mem_order:
        assert start[j] == pos
        assert (off_all[pos:pos + c.ns[j]] == offs[j]).all() and (len_all[pos:pos + c.ns[j]] == c.lens[j]).all()
        pos += c.ns[j]
    assert len(off_all) == len(len_all) == pos + mc.TAIL and mc.TAIL == 3 * 64
    assert not off_all[pos:].any() and (len_all[pos:] == 64).all()
    assert pool[:64].tobytes() == mc.SPARE and (pool.size % 64) == 0
    assert all(int(o.min()) >= 1 for o in offs if len(o))
    # every descriptor names a whole frame inside its pool, in both forms
    sp = c.strided
    assert sp[:64].tobytes() == mc.SPARE
    seen = np.zeros(sp.size // 64, dtype=bool)
    seen[0] = True
    for j in range(c.k):
        for i, f in enumerate(c.frames(j)):
            a = int(offs[j][i]) * 64
            assert pool[a:a + len(f)].tobytes() == f
            s = c.slot0(j) + i * c.stride64
            assert sp[s * 64:s * 64 + len(f)].tobytes() == f
            assert len(f) <= 64 * c.stride64 // c.k or (len(f) == 1500 and (j, i) == (c.k - 1, max(c.ns) - 1))
            assert (sp[s * 64 + len(f):(s + (len(f) + 63) // 64) * 64] == mc.FILL).all()
            seen[s:s + (len(f) + 63) // 64] = True
    assert (sp.reshape(-1, 64)[~seen] == mc.FILL).all()
    assert c.stride64 == (2 if c.wide else 1) * c.k and [c.slot0(j) for j in range(c.k)] == \
        [1 + (2 if c.wide else 1) * j for j in range(c.k)]
    # records: GUARD records behind every burst, the whole buffer accounted for, REC8 off 16
    for kind in KINDS:
        where, size = c.rec_layout(kind)
        imgs, _ = c.expect(kind)
        spans = [[] for _ in size]
        for j in range(c.k):
            b, o = where[j]
            assert o % (8 if kind == rxg.REC8 else 16) == 0
            spans[b].append((o, o + c.ns[j] * kind))
        for b, sp_ in enumerate(spans):
            sp_.sort()
            lead = 8 if kind == rxg.REC8 else 0
            assert sp_[0][0] == lead and (imgs[b][:lead] == mc.FILL).all()
            for (a0, a1), (b0, _) in zip(sp_, sp_[1:] + [(size[b], None)]):
                assert b0 - a1 == mc.GUARD * kind and (imgs[b][a1:b0] == mc.FILL).all()
        if kind == rxg.REC8 and sum(c.ns):
            assert any(where[j][1] % 16 == 8 for j in range(c.k) if c.ns[j]), "no REC8 burst off 16-byte alignment"
        assert len(size) == (2 if c.split else 1)


def test_every_launch_is_a_few_thousand_frames():
    for name in mc.ALL:
        assert all(sum(l.n) <= 4200 for l in mc.get(name).launches), name


# ----------------------------------------------------------------------------------- model ---
def test_model_numbering_grid_and_depth():
    ls = mc.plan([0, 65, 0, 0, 1, 129, 0])
    assert len(ls) == 1 and ls[0].caller == [1, 4, 5] and ls[0].slice0 == [0, 2, 3] and ls[0].nslices == 6
    assert ls[0].multi and ls[0].blocks(1) == 1 and ls[0].blocks(2) == 2 and ls[0].blocks(768) == 2
    assert mc.plan([0] * 40) == [] and [l.caller for l in mc.plan([0] * 32 + [5])] == [[32]]
    assert [len(l.n) for l in mc.plan([1] * 97)] == [32, 32, 32, 1]
    big = mc.plan([64 * 64])[0]
    assert big.nslices == 64 and big.deep(1, 8) and big.deep(1, 16) and not big.deep(1, 48) and not big.deep(2, 8)
    assert not mc.plan([64 * 63])[0].deep(1, 8) and mc.plan([64 * 128])[0].deep(2, 16)
    assert list(mc.wave_slices(10, 1, 1)) == [1, 5, 9] and list(mc.wave_slices(10, 2, 7)) == [7]
    # the ring: slots a slice's scratch asks for, per kind and path
    assert [mc.need_slots(k, True) for k in KINDS] == [8, 4, 2]
    assert [mc.need_slots(k, False) for k in KINDS] == [11, 6, 3]
    for k in KINDS:      # rx_body's static_assert: the ring holds either scratch and one record
        assert mc.RS[k] > mc.need_slots(k, True) and mc.RS[k] >= mc.need_slots(k, False)


# ----------------------------------------------------------------------------------- pairs ---
def test_pairs():
    assert len(mc.PAIR_WALK) == 26 and mc.PAIR_WALK[0] == mc.PAIR_WALK[-1]
    assert set(zip(mc.PAIR_WALK, mc.PAIR_WALK[1:])) == {(a, b) for a in mc.SIZES for b in mc.SIZES}
    for name in mc.NAMES["pairs"]:
        c = mc.get(name)
        assert c.ns == mc.PAIR_WALK and len(c.launches) == 1 and c.launches[0].multi
        sl = sl_of(c, c.launches[0])
        for w in range(mc.WAVES):      # one workgroup: every wave walks through at least five bursts
            assert len({sl[s].k for s in mc.wave_slices(len(sl), 1, w)}) >= 5
        for blocks in CAPPED:
            assert not c.launches[0].deep(blocks, rxg.REC8)
    c = mc.get("pairs/big_last")
    sl = sl_of(c, c.launches[0])
    for j in range(c.k):
        assert c.lens[j][-1] == mc.BIG and all(ln <= 64 for ln in c.lens[j][:-1])
        assert not [s for s in sl if s.j == j][-1].small
    assert all(s.small == (s.frames == 64) for s in sl_of(mc.get("pairs/small"), mc.get("pairs/small").launches[0]))


# --------------------------------------------------------------------------------- empties ---
def test_empties():
    pats = mc.EMPTY_PATTERNS
    assert pats["first"] == [0] and pats["last"] == [mc.EMPTY_K - 1]
    mid = pats["two_mid"]
    assert len(mid) == 2 and mid[1] == mid[0] + 1 and 0 < mid[0] and mid[1] < mc.EMPTY_K - 1
    assert [next(j for j in range(6) if j not in pats[p]) for p in ("only_0", "only_3", "only_5")] == [0, 3, 5]
    assert all(len(pats[p]) == 5 for p in ("only_0", "only_3", "only_5")) and len(pats["all"]) == 6
    for p, hole in pats.items():
        for v in ("valid", "null"):
            c = mc.get(f"empties/{p}/{v}")
            assert c.k == 6 and [j for j in range(6) if not c.ns[j]] == hole and c.null_empties == (v == "null")
            if p == "all":
                assert c.launches == []
                continue
            (l,) = c.launches
            assert l.caller == [j for j in range(6) if j not in hole]
            assert l.multi == (len(hole) < 5)
    # the non-MULTI kernel on a burst that is not the caller's bursts[0]
    assert [mc.get(f"empties/{p}/null").launches[0].caller for p in ("only_3", "only_5")] == [[3], [5]]
    # a partial last slice, a one-frame burst and full slices among the bursts that stay
    assert {n % 64 for n in mc.EMPTY_FULL} >= {0, 1, 63} and 1 in mc.EMPTY_FULL


# ---------------------------------------------------------------------------------- counts ---
def test_counts():
    assert mc.COUNT_KS == [1, 2, 31, 32, 33, 63, 64, 65, 97] and mc.COUNT_NS == [1, 65]
    for n in mc.COUNT_NS:
        for k in mc.COUNT_KS:
            c = mc.get(f"counts/{k}/{n}")
            assert c.ns == [n] * k
            assert [len(l.n) for l in c.launches] == [32] * (k // 32) + ([k % 32] if k % 32 else [])
            assert [l.multi for l in c.launches] == [len(l.n) > 1 for l in c.launches]
            if n == 1:      # one valid lane per slice
                assert all(s.frames == 1 for l in c.launches for s in sl_of(c, l))
    assert mc.get("counts/32/1").launches[0].slice0[31] == 31      # the lookup reads lane 31
    for k in (33, 65):
        assert not mc.get(f"counts/{k}/65").launches[-1].multi and mc.get(f"counts/{k}/1").launches[-1].n == [1]
    assert len(mc.get("counts/97/1").launches) == 4
    a, b, x = (mc.get(f"counts/{h}") for h in mc.COUNT_HOLES)
    assert a.k == b.k == 64 and x.k == 40
    assert [l.caller for l in a.launches] == [list(range(32, 64))]      # only the second launch is made
    assert [l.caller for l in b.launches] == [list(range(32))]
    assert [l.caller for l in x.launches] == [list(range(30)), list(range(34, 40))]
    assert [j for j in range(40) if not x.ns[j]] == [30, 31, 32, 33]


# ------------------------------------------------------------------------------------ ring ---
def ring_findings():
    """(kind, deep?) -> [early flush of >= 2 bursts seen, one holding a burst's partial last slice
    seen], over the ring sets on the capped grids."""
    found = {}
    for name in mc.NAMES["ring"]:
        c = mc.get(name)
        (l,) = c.launches
        sl = sl_of(c, l)
        for blocks in CAPPED:
            for kind in KINDS:
                f = found.setdefault((kind, l.deep(blocks, kind)), [False, False])
                for wave in mc.flushes(sl, kind, l.blocks(blocks)):
                    for slots, final in wave:
                        if not final and len({s.k for s in slots}) >= 2:
                            f[0] = True
                            f[1] |= any(s.last_partial for s in slots)
    return found


def test_ring():
    a, b, c32, c31 = (mc.get(n) for n in mc.NAMES["ring"])
    assert a.ns == b.ns == [129] * 32 and c32.ns == [65] * 32 and c31.ns == [65] * 31
    assert a.launches[0].nslices == 96 and c32.launches[0].nslices == 64 and c31.launches[0].nslices == 62
    assert all(s.small == (s.frames == 64) for s in sl_of(a, a.launches[0]))
    sb = sl_of(b, b.launches[0])
    assert not any(s.small for s in sb) and all(len(s.big) == 1 for s in sb)      # every slice on the class path
    assert sorted({ln for x in b.lens for ln in x if ln > 64}) == [100, 1500] and b.lens[31][128] == 1500
    # 24 and 16 slices per wave on one workgroup take the DEEP kernels, one burst fewer the plain ones
    for kind in (rxg.REC8, rxg.REC16):
        assert a.launches[0].deep(1, kind) and c32.launches[0].deep(1, kind)
        assert not c31.launches[0].deep(1, kind) and not a.launches[0].deep(2, kind)
    found = ring_findings()
    for kind in KINDS:
        for deep in (False, True):
            if deep and kind in mc.NEVER_DEEP:
                assert (kind, deep) not in found, "REC48 has no DEEP kernel (launch_rx): nothing to reach"
                continue
            assert found[(kind, deep)] == [True, True], \
                f"REC{kind} {'DEEP' if deep else 'plain'}: no early flush with slots of two bursts / a partial last slice"


def test_ring_flush_model_on_a_known_wave():
    """ring/x31_65 on one workgroup, REC8: wave 0 takes the 16 full slices 0, 4, .. 60 (flush of 15
    at the 16th, RS 22 less 8 scratch slots), wave 1 the 16 one-frame slices (flush of 12, 11
    scratch slots on the class path)."""
    c = mc.get("ring/x31_65")
    fl = mc.flushes(sl_of(c, c.launches[0]), rxg.REC8, 1)
    assert [(len(s), f) for s, f in fl[0]] == [(15, False), (1, True)]
    assert [(len(s), f) for s, f in fl[1]] == [(12, False), (4, True)]
    assert all(s.frames == 1 for s in fl[1][0][0]) and len({s.k for s in fl[1][0][0]}) == 12
    assert sum(len(s) for w in fl for s, _ in w) == 62


# ------------------------------------------------------------------------------------ runs ---
def test_runs_short():
    c = mc.get("runs/short")
    (l,) = c.launches
    assert l.nslices < 64 and not l.deep(1, rxg.REC8) and l.blocks(1) == 1
    ev = mc.run_events(sl_of(c, l), 1, deep=False)
    assert {e[1] for e in ev} == {"d1"}
    for what in mc.RUN_KINDS:      # the look-ahead lands in the next burst each time (or past the launch)
        assert any(e[2] == what and (e[3] or what == "past") for e in ev), what
    where = {what: {e[0] for e in ev if e[2] == what} for what in mc.RUN_KINDS}
    # five conditions on four waves: the four that end a run inside the launch on a wave each
    assert [where[w] for w in ("partial", "big0", "one", "big63")] == [{1}, {2}, {3}, {0}]
    assert where["full"] == where["past"] == {0, 1, 2, 3}
    assert "other" not in {e[2] for e in ev}


def test_runs_deep():
    c = mc.get("runs/deep")
    (l,) = c.launches
    assert l.nslices >= 64 and l.deep(1, rxg.REC8) and l.deep(1, rxg.REC16) and len(l.n) <= mc.K_MAX_BURSTS
    assert all(n == 256 for n in c.ns[:12])                     # full small bursts in front
    sl = sl_of(c, l)
    ev = mc.run_events(sl, 1, deep=True)
    for where in ("entry", "d2"):      # one slice ahead at a run's start; two ahead with pend set
        for what in mc.RUN_KINDS:
            assert any(e[1] == where and e[2] == what and (e[3] or what == "past") for e in ev), (where, what)
    # s + nwaves ends the run while s + 2 nwaves is all small (pend clear), behind every kind of end
    for what in ("partial", "big0", "big63", "one"):
        starts = {(e[0], e[4]) for e in ev if e[1] == "entry" and e[2] == what}
        assert any(e[1] == "d2clear" and e[2] == "full" and (e[0], e[4]) in starts for e in ev), what
    by_wave = {what: {e[0] for e in ev if e[1] == "d2" and e[2] == what} for what in mc.RUN_KINDS}
    assert [by_wave[w] for w in ("partial", "big0", "big63", "one")] == [{0}, {1}, {2}, {3}]
    assert "other" not in {e[2] for e in ev}
    # on the plain kernel (REC48, or two workgroups) the same launch is one-deep
    assert not l.deep(1, rxg.REC48) and not l.deep(2, rxg.REC8)


# ----------------------------------------------------------------------------------- order ---
def test_order():
    for name in mc.NAMES["order"]:
        c = mc.get(name)
        assert c.ns == mc.PAIR_WALK and c.mem_order == list(range(25, -1, -1))
        _, _, start = c.desc
        assert all(start[j] > start[j + 1] or c.ns[j + 1] == 0 for j in range(c.k - 1))      # burst 25 first
        for kind in KINDS:
            where, size = c.rec_layout(kind)
            for b in range(len(size)):
                at = [where[j][1] for j in range(c.k) if where[j][0] == b]
                assert at == sorted(at, reverse=True)
            assert [where[j][0] for j in range(c.k)] == ([j % 2 for j in range(c.k)] if c.split else [0] * c.k)
    assert mc.get("order/split").split and not mc.get("order/reversed").split
    assert mc.get("order/reversed").oracle[0].tobytes() == mc.get("pairs/small").oracle[0].tobytes()


def test_names():
    assert mc.ALL == [n for s in ("pairs", "empties", "counts", "ring", "runs", "order") for n in mc.NAMES[s]]
    assert mc.WITH_REC48 == ("pairs", "ring", "counts")
    assert pktgen.ESTABLISHED == rxg.TCP_ESTABLISHED
