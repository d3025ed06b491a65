"""GPU: rxg_flow_trains_dev (a burst's data segments grouped by flow and cut into trains on the
device) and the trains' use during the replay (rxg_flow_trains_attach / rxg_flow_train_current)
against the numpy model tests/flowtrain_ref.py -- never against the kernels' own output or the
host function alone.  Records are crafted in all three layouts with every bit outside the decoded
fields random (tests/flowtrain_cases.py; its claims are asserted in tests/test_flowtrain_host.py);
one test ties the reader of those layouts to a real rxg_rx_burst_dev's records.  Outputs are
pre-filled with 0xA5 and compared whole, eight guard entries behind `order` and `trains` and the
words around `count` included."""
import ctypes as C

import numpy as np
import pytest

import flowsum_cases as fcases
import flowtrain_cases as cases
import flowtrain_ref as ref
import oracle
import pktgen
import rxg
from test_gpu_replay import Model, scenario, sequential_reference

pytestmark = pytest.mark.gpu

FILL, GUARD, EINVAL = 0xA5, 8, 22
FILL64 = 0xA5A5A5A5A5A5A5A5
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
TILE = cases.TILE


class Batch:
    """A burst's records (and frames) on the device with the model's answer for them."""

    def __init__(self, eng, rec_kind, ntcb, recs, frames=None, flags=0, cur=None, strided=False):
        self.eng, self.rec_kind, self.ntcb, self.flags, self.cur = eng, rec_kind, ntcb, flags, cur
        self.dev = []
        self.n = len(recs) // rec_kind
        self.da = self.do = self.dl = self.dc = None
        self.geom = None
        if frames is not None:
            lens = np.array([len(f) for f in frames], np.uint16)
            if strided:
                stride64 = max(1, (int(lens.max()) + 63) // 64)
                off = (5 + np.arange(self.n) * stride64).astype(np.uint32)
                arena = np.full((5 + self.n * stride64) * 64, 0x5C, np.uint8)
                for f, o in zip(frames, off.tolist()):
                    arena[o * 64:o * 64 + len(f)] = np.frombuffer(f, np.uint8)
                self.geom = (5, stride64)
            else:
                arena, off, lens = pktgen.pack_arena(frames)
            self.da, self.do, self.dl = self.up(arena), self.up(off), self.up(lens)
        self.dr = self.up(recs)
        if cur is not None:
            self.dc = self.up(cur)
        self.worder, self.wtrains, self.wcount = ref.trains(recs, rec_kind, ntcb, frames, flags, cur)
        self.S, self.T = len(self.worder), len(self.wtrains)

    @classmethod
    def of(cls, eng, case, rec_kind, **kw):
        return cls(eng, rec_kind, case.ntcb, case.records(rec_kind), None if rec_kind == rxg.REC48 else case.frames(),
                   case.flags, case.cur_array(), **kw)

    def up(self, a):
        d = self.eng.to_device(np.ascontiguousarray(a).view(np.uint8) if len(a) else np.zeros(16, np.uint8))
        self.dev.append(d)
        return d

    def outs(self, cap_seg=None, cap_trains=None):
        cap_seg = self.S if cap_seg is None else cap_seg
        cap_trains = self.T if cap_trains is None else cap_trains
        return (self.eng.to_device(np.full((cap_seg + GUARD) * 4, FILL, np.uint8)),
                self.eng.to_device(np.full((cap_trains + GUARD) * 32, FILL, np.uint8)),
                self.eng.to_device(np.full(6 * 8, FILL, np.uint8)), cap_seg, cap_trains)

    def call(self, eng, o, stream=None, use_stride=False):
        order, trains, count, cap_seg, cap_trains = o
        eng.flow_trains_dev(self.dr.ptr, self.rec_kind, self.n, self.ntcb, order.ptr, cap_seg, trains.ptr, cap_trains,
                            count.ptr + 8, cur_seq=None if self.dc is None else self.dc.ptr,
                            frames=None if self.da is None else self.da.ptr, lens=None if self.dl is None else self.dl.ptr,
                            off64=None if (use_stride or self.do is None) else self.do.ptr,
                            slot0=self.geom[0] if use_stride else 0, stride64=self.geom[1] if use_stride else 0,
                            flags=self.flags, stream=stream)

    def check(self, o, what=""):
        order, trains, count, cap_seg, cap_trains = o
        cw = count.download(np.uint64, 6)
        assert cw[0] == cw[5] == FILL64, (what, "words around count were written")
        assert cw[1:5].tolist() == self.wcount.tolist(), (what, cw[1:5], self.wcount)
        go = order.download(np.uint32, cap_seg + GUARD)
        gt = trains.download(np.uint8, (cap_trains + GUARD) * 32).view(rxg.FLOW_TRAIN_DTYPE)
        s, t = min(self.S, cap_seg), min(self.T, cap_trains)
        if go[:s].tobytes() != self.worder[:s].tobytes():
            bad = np.nonzero(go[:s] != self.worder[:s])[0]
            raise AssertionError(f"{what}: {len(bad)} of {s} order entries differ, first at {bad[0]}: got {go[bad[0]]} "
                                 f"want {self.worder[bad[0]]}")
        assert (go[s:] == 0xA5A5A5A5).all(), (what, "order written at or past min(S, cap_seg)")
        if gt[:t].tobytes() != self.wtrains[:t].tobytes():
            bad = [i for i in range(t) if gt[i] != self.wtrains[i]]
            raise AssertionError(f"{what}: {len(bad)} of {t} trains differ, first at {bad[0]}: got {gt[bad[0]]} want "
                                 f"{self.wtrains[bad[0]]}")
        assert (gt[t:].view(np.uint8) == FILL).all(), (what, "trains written at or past min(T, cap_trains)")
        return go[:s].tobytes() + gt[:t].tobytes() + cw[1:5].tobytes()

    def run(self, eng=None, what="", cap_seg=None, cap_trains=None, **kw):
        eng = eng or self.eng
        o = self.outs(cap_seg, cap_trains)
        try:
            self.call(eng, o, **kw)
            eng.sync()
            return self.check(o, what)
        finally:
            free(o)

    def close(self):
        for d in self.dev:
            d.free()


def free(o):
    for d in o[:3]:
        d.free()


@pytest.fixture(scope="module")
def capped():
    engs = [rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)]
    yield engs
    for e in engs:
        e.close()


# ------------------------------------- 1. every case set, every layout, three grids ---
SMALL = {c.name: c for c in cases.rule_cases()}


@pytest.mark.parametrize("name", list(SMALL))
def test_case_sets_in_every_layout_and_on_capped_grids(engine, capped, name):
    case = SMALL[name]
    for k, kind in enumerate(KINDS):
        b = Batch.of(engine, case, kind, strided=(kind == rxg.REC16))
        try:
            a = b.run(what=f"{name}, records of {kind}", use_stride=(kind == rxg.REC16))
            assert a == b.run(capped[0], what=f"{name}, records of {kind}, max_blocks 1")
            assert a == b.run(capped[1], what=f"{name}, records of {kind}, max_blocks 2")
        finally:
            b.close()


def test_reader_of_the_layouts_on_a_real_burst(engine):
    """Records written by rxg_rx_burst_dev itself, in each kind, frames through off64 and a stride."""
    rng = np.random.default_rng(21)
    rows = fcases.table(40)
    flow_of = np.where(rng.random(1500) < 0.1, -1, np.repeat(rng.integers(0, 40, 1500 // 4 + 1), 4)[:1500])
    frames, nxt = [], {}
    r2 = np.random.default_rng(5)
    for f in flow_of.tolist():
        if f < 0:
            frames.append(pktgen.frame(src_ip=pktgen.ip4(172, 16, 1, 9), dst_ip=fcases.DST, sport=40000, dport=9999, flags=0x10))
            continue
        seq = nxt.get(f, int(r2.integers(1, 1 << 32))) if r2.random() < 0.8 else int(r2.integers(1, 1 << 32))
        pay = r2.bytes(int(r2.integers(0, 200)))
        fl = 0x11 if r2.random() < 0.03 else 0x10
        frames.append(fcases.flow_frame(f, seq, 1, fl, pay))
        nxt[f] = (seq + len(pay)) & 0xFFFFFFFF
    arena, off, lens = pktgen.pack_arena(frames)
    tcb, live = pktgen.table_arrays(rows)
    engine.tcb_load(tcb, live)
    want48 = oracle.rx_batch(arena, off, lens, tcb, live)[0]
    da, do, dl = engine.to_device(arena), engine.to_device(off.view(np.uint8)), engine.to_device(lens.view(np.uint8))
    try:
        for kind in KINDS:
            dr = engine.to_device(np.full(len(frames) * kind, FILL, np.uint8))
            engine.rx_burst_dev(da.ptr, do.ptr, dl.ptr, len(frames), dr.ptr, kind)
            engine.sync()
            recs = dr.download(np.uint8, len(frames) * kind)
            dr.free()
            assert recs.tobytes() == np.ascontiguousarray(fcases.as_kind(want48, kind)).tobytes()
            cur = np.zeros(len(rows), np.uint32)
            for f in range(0, 40, 2):
                first = next((fr for fr, g in zip(frames, flow_of.tolist()) if g == f and len(fr) > 54), None)
                if first:
                    cur[f] = int.from_bytes(first[38:42], "big")
            b = Batch(engine, kind, len(rows), recs, frames, cur=cur)
            try:
                assert b.T > 100 and int((b.wtrains["nseg"] > 2).sum()) > 20
                assert int(((b.wtrains["flags"] & rxg.FTR_HEAD) != 0).sum()) > 10
                dev = b.run(what=f"a real burst, records of {kind}")
                order, trains, count = rxg.flow_trains_host(recs, kind, len(rows), frames, cur_seq=cur)
                assert order.tobytes() + trains.tobytes() + count.tobytes() == dev       # host and device agree
            finally:
                b.close()
    finally:
        for d in (da, do, dl):
            d.free()


# ----------------------------------------------------------------- 2. scan edges ---
@pytest.mark.parametrize("n", cases.SCAN_SIZES)
def test_scan_round_edges_on_three_grids(engine, capped, n):
    """Frame counts one tile (slice) below, at and one frame above a round of a sort pass's scan
    (of the select's scan), all frames segments.  (A round of the cut's scan is 2^24 frames.)"""
    r = cases.big(n, seed=n)
    b = Batch(engine, rxg.REC48, 1000, np.ascontiguousarray(r).view(np.uint8))
    try:
        assert b.S == n and n // 64 * 0.4 < b.T < n // 64 + 2
        a = b.run(what=f"{n} segments")
        assert a == b.run(capped[0], what=f"{n} segments, max_blocks 1")
        assert a == b.run(capped[1], what=f"{n} segments, max_blocks 2")
    finally:
        b.close()


# ----------------------------------------------------------------------- 3. caps ---
def test_caps_and_no_state_between_calls(engine):
    import torch
    s = torch.cuda.Stream()
    small = Batch.of(engine, SMALL["gap, overlap, duplicate"], rxg.REC16)
    mid = Batch.of(engine, SMALL[f"mixed, {2 * TILE + 1} frames"], rxg.REC8)
    r = cases.big(5 * TILE + 3, nflows=300, run=7, seed=9)
    large = Batch(engine, rxg.REC48, 70000, np.ascontiguousarray(r).view(np.uint8))
    try:
        for b in (small, mid, large):
            S, T = b.S, b.T
            assert S > 2 and T > 2
            for cap_seg, cap_trains in ((0, T), (S, 0), (S - 1, T), (S, T - 1), (S // 2, T // 2), (0, 0), (S, T)):
                b.run(cap_seg=cap_seg, cap_trains=cap_trains, what=f"caps {cap_seg} {cap_trains} of {S} {T}")
        large.run(what="the largest")
        small.run(what="a small call after a larger one")       # the scratch carries nothing over
        mid.run(what="and a middle one")
        # no host wait between calls, and calls on another stream in between
        outs = [small.outs(), large.outs(), mid.outs(), small.outs()]
        small.call(engine, outs[0])
        large.call(engine, outs[1], stream=s.cuda_stream)
        mid.call(engine, outs[2])
        small.call(engine, outs[3], stream=s.cuda_stream)
        engine.sync()
        engine.stream_sync(s.cuda_stream)
        for b, o, what in ((small, outs[0], "first"), (large, outs[1], "caller stream"), (mid, outs[2], "third"),
                           (small, outs[3], "caller stream again")):
            b.check(o, what)
        for o in outs:
            free(o)
    finally:
        for b in (small, mid, large):
            b.close()


# ----------------------------------------------------- 4. n == 0 and argument errors ---
def test_argument_errors_and_empty_bursts_write_nothing(engine):
    lib = rxg.load_library()
    b = Batch.of(engine, SMALL["FIN in the middle and at the end"], rxg.REC16)
    o = b.outs()
    order, trains, count, cap_seg, cap_trains = o
    try:
        def args(**kw):
            a = dict(frames=b.da.ptr, off64=b.do.ptr, len=b.dl.ptr, slot0=0, stride64=0, n=b.n, rec_kind=b.rec_kind,
                     recs=b.dr.ptr, ntcb=b.ntcb, flags=0, cur_seq=b.dc.ptr, order=order.ptr, cap_seg=cap_seg,
                     trains=trains.ptr, cap_trains=cap_trains, count=count.ptr + 8)
            a.update(kw)
            return rxg.DevFlowTrains(**a)
        bad = [(dict(recs=None), b"NULL"), (dict(count=None), b"NULL"), (dict(order=None), b"NULL"),
               (dict(trains=None), b"NULL"), (dict(frames=None), b"NULL"), (dict(len=None), b"NULL"),
               (dict(rec_kind=0), b"rec_kind"), (dict(rec_kind=32), b"rec_kind"),
               (dict(ntcb=0), b"ntcb"), (dict(ntcb=rxg.FS_MAX_NTCB + 1), b"ntcb"),
               (dict(flags=2), b"flags"), (dict(flags=0x80000001), b"flags"),
               (dict(frames=b.da.ptr + 8), b"alignment"), (dict(trains=trains.ptr + 4), b"alignment"),
               (dict(count=count.ptr + 12), b"alignment"), (dict(off64=b.do.ptr + 2), b"alignment"),
               (dict(order=order.ptr + 2), b"alignment"), (dict(cur_seq=b.dc.ptr + 2), b"alignment"),
               (dict(len=b.dl.ptr + 1), b"alignment"), (dict(recs=b.dr.ptr + 8), b"alignment"),
               (dict(recs=b.dr.ptr + 4, rec_kind=rxg.REC8), b"alignment"),
               (dict(off64=None, stride64=0), b"stride64"),
               (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
               (dict(off64=None, slot0=0, stride64=0xFFFFFFFF, n=3), b"2^32")]
        for kw, why in bad:
            assert lib.rxg_flow_trains_dev(engine.ctx, C.byref(args(**kw)), None) == -EINVAL, kw
            assert why in lib.rxg_last_error(), (kw, lib.rxg_last_error())
        assert lib.rxg_flow_trains_dev(engine.ctx, None, None) == -EINVAL
        assert lib.rxg_flow_trains_dev(None, C.byref(args()), None) == -EINVAL
        engine.sync()

        def untouched():
            return ((order.download(np.uint8, (cap_seg + GUARD) * 4) == FILL).all() and
                    (trains.download(np.uint8, (cap_trains + GUARD) * 32) == FILL).all())
        assert untouched() and (count.download(np.uint8, 48) == FILL).all()
        # n == 0: count = {0, 0, 0, 0} and nothing else, in either addressing mode; NULL outputs with cap 0 are fine
        for kw in (dict(n=0), dict(n=0, off64=None, stride64=4),
                   dict(n=0, order=None, cap_seg=0, trains=None, cap_trains=0, cur_seq=None)):
            assert lib.rxg_flow_trains_dev(engine.ctx, C.byref(args(**kw)), None) == 0, lib.rxg_last_error()
            engine.sync()
            assert count.download(np.uint64, 6).tolist() == [FILL64, 0, 0, 0, 0, FILL64]
            assert untouched()
            count.upload(np.full(48, FILL, np.uint8))
        # and the valid call works
        assert lib.rxg_flow_trains_dev(engine.ctx, C.byref(args()), None) == 0
        engine.sync()
        b.check(o)
    finally:
        free(o)
        b.close()


# --------------------------------------------------------------------- 5. the replay ---
def continuing(frames, p_cont=0.75, seed=3):
    """The scenario's frames with the established flows' segments (10.1.x.y -> port 80) given
    continuing sequence numbers: each follows its flow's previous frame with probability p_cont.
    Everything else of a frame stays (tuple, flags, ack, payload); checksums are filled again."""
    rng = np.random.default_rng(seed)
    out, nxt = [], {}
    for f in frames:
        src, sport = int.from_bytes(f[26:30], "big"), int.from_bytes(f[34:36], "big")
        if src >> 16 != (10 << 8 | 1) or len(f) < 54:
            out.append(f)
            continue
        key, pay = (src, sport, int.from_bytes(f[36:38], "big")), f[54:]
        seq = nxt[key] if key in nxt and rng.random() < p_cont else int.from_bytes(f[38:42], "big")
        out.append(pktgen.frame(src_ip=src, dst_ip=int.from_bytes(f[30:34], "big"), sport=sport, dport=key[2], seq=seq,
                                ack=int.from_bytes(f[42:46], "big"), flags=f[47], payload=pay))
        assert len(out[-1]) == len(f)
        nxt[key] = (seq + len(pay)) & 0xFFFFFFFF
    return out


def run_replay(eng, rows, frames, recs, ask):
    """The replay with the model's handlers; ask(i) runs inside tcpswitch and inside send_reset
    for packet i (a segment the replay re-classified to a reset reaches only the latter)."""
    lib = rxg.load_library()
    bufs = [C.create_string_buffer(f, max(len(f), 64)) for f in frames]
    addr = {C.addressof(x): i for i, x in enumerate(bufs)}
    model = Model(rows, eng)

    def switch(u, idx, st, tcp, ip, m):
        ask(addr[m])
        model.handle(idx, st, frames[addr[m]])
        return 0

    def reset(u, ip, tcp):                                  # (the frame's IPv4 header, at byte 14)
        ask(addr[ip - 14])

    ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(), rxg.HANDOFF_ADD_MAC(),
                         rxg.HANDOFF_SEND_RESET(reset), rxg.HANDOFF_ON_SEGMENT(), rxg.HANDOFF_TCPSWITCH(switch))
    ptrs = (C.c_void_p * len(bufs))(*[C.addressof(x) for x in bufs])
    rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, len(bufs), 16)
    assert rc == 0, lib.rxg_last_error()
    return model


def replay_case():
    """The seeded scenario with continuing flows: its frames, the sequential reference's answers,
    the burst's records, the model's trains and the caps the test attaches with.  cap_seg ends
    one segment short of the end of the last train of several segments, so that train -- and
    every later one -- is in `trains` but not whole inside `order`; cap_trains leaves out the
    last train."""
    rows, frames = scenario(5, n=900)
    frames = continuing(frames)
    exp, _, erows = sequential_reference(rows, frames)
    arena, off, lens = pktgen.pack_arena(frames)
    tcb, live = pktgen.table_arrays(rows)
    recs16 = np.ascontiguousarray(oracle.rx_batch(arena, off, lens, tcb, live)[0]["c"])
    worder, wtrains, wcount = ref.trains(recs16.view(np.uint8), rxg.REC16, len(rows), frames)
    S, T = len(worder), len(wtrains)
    cut = wtrains[np.nonzero(wtrains["nseg"] > 1)[0][-1]]          # the train order is capped inside
    cap_seg, cap_trains = int(cut["first"]) + int(cut["nseg"]) - 1, T - 1
    where, capped = {}, set()
    for k, t in enumerate(wtrains):
        seg = worder[int(t["first"]):int(t["first"]) + int(t["nseg"])].tolist()
        if k < cap_trains and int(t["first"]) + int(t["nseg"]) <= cap_seg:
            where.update({i: (k, p) for p, i in enumerate(seg)})
        else:
            capped.update(seg)
    changed = {i for i, (v, idx, st) in enumerate(exp)
               if (v, idx, st) != (int(recs16["verdict"][i]), int(recs16["tcb_idx"][i]), int(recs16["state"][i]))}
    return dict(rows=rows, frames=frames, exp=exp, erows=erows, recs16=recs16, worder=worder, wtrains=wtrains,
                cap_seg=cap_seg, cap_trains=cap_trains, where=where, capped=capped, changed=changed, cut=cut)


def test_replay_names_the_models_train_and_position(replay_engine):
    eng = replay_engine
    lib = rxg.load_library()
    rc = replay_case()
    rows, frames, recs16, where, changed, capped = (rc[k] for k in ("rows", "frames", "recs16", "where", "changed", "capped"))
    n = len(frames)
    # what the case must hold for the checks below to mean anything
    multi = {i for i, (k, p) in where.items() if int(rc["wtrains"][k]["nseg"]) > 1}
    later = {i for i, (k, p) in where.items() if p > 0}
    assert len(later) > 40 and int(rc["wtrains"]["nseg"].max()) >= 4
    assert len(changed & set(where)) > 3 and len(changed & later) > 0       # re-classified segments, not all first
    cut_seg = rc["worder"][int(rc["cut"]["first"]):int(rc["cut"]["first"]) + int(rc["cut"]["nseg"])].tolist()
    assert set(cut_seg) <= capped and len(cut_seg) > 1 and rc["cap_seg"] > int(rc["cut"]["first"])
    eng.tcb_load(*pktgen.table_arrays(rows))
    b = Batch(eng, rxg.REC16, len(rows), recs16.view(np.uint8), frames)
    o = b.outs(cap_seg=rc["cap_seg"], cap_trains=rc["cap_trains"])
    try:
        assert b.worder.tolist() == rc["worder"].tolist()
        eng.rx_burst_dev(b.da.ptr, b.do.ptr, b.dl.ptr, n, b.dr.ptr, rxg.REC16)    # the burst the replay replays
        b.call(eng, o)
        eng.sync()
        b.check(o)
        order = o[0].download(np.uint32, rc["cap_seg"]).copy()
        trains = o[1].download(np.uint8, rc["cap_trains"] * 32).view(rxg.FLOW_TRAIN_DTYPE).copy()
        recs = b.dr.download(rxg.REC16_DTYPE, n)
        assert recs.tobytes() == recs16.tobytes()
        assert eng.flow_train_current() is None                # before the replay: nothing
        eng.flow_trains_attach(order.ctypes.data, len(order), trains.ctypes.data, len(trains))
        assert eng.flow_train_current() is None                # attached, but no replay runs
        seen = {}
        model = run_replay(eng, rows, frames, recs, lambda i: seen.__setitem__(i, eng.flow_train_current()))
        assert model.rows == rc["erows"]
        ones, deep, last, refused_changed, refused_capped = 0, 0, 0, 0, 0
        for i, got in seen.items():
            if i in changed or i not in where:
                assert got is None, i
                refused_changed += i in changed and i in where
                refused_capped += i in capped
            elif got is not None:
                t, pos = got
                k, p = where[i]
                assert pos == p and t == b.wtrains[k] and int(order[int(t["first"]) + pos]) == i, (i, pos, p)
                ones += 1
                deep += pos > 0
                last += pos > 0 and pos + 1 == int(t["nseg"])
            else:
                # an unchanged answer may still have been re-classified (its tuple was written): then 0
                assert int(rxg_stats(eng)[0]) > 0, i
        assert ones > 60 and deep > 30 and last > 10           # positions past 0, trains' last segments among them
        assert refused_changed > 0                              # a re-classified segment of an attached train asked, got 0
        assert refused_capped > 0 and any(i in seen for i in cut_seg[1:])     # and a capped train's later segment
        assert any(i in seen and i in later for i in changed)
        assert eng.flow_train_current() is None                # the attachment ended with the replay
        p, k = C.c_void_p(), C.c_uint32()
        assert lib.rxg_flow_train_current(eng.ctx, None, C.byref(k)) == -EINVAL
        assert lib.rxg_flow_train_current(eng.ctx, C.byref(p), None) == -EINVAL
        assert lib.rxg_flow_train_current(None, C.byref(p), C.byref(k)) == -EINVAL
        # attach refuses lists that do not tile [0, nseg) in order, and NULLs
        swapped = trains.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        holed = trains.copy()
        holed["first"][3] += 1
        empty = trains.copy()
        empty["nseg"][2] = 0
        for t in (swapped, holed, empty, trains[1:].copy()):
            assert lib.rxg_flow_trains_attach(eng.ctx, order.ctypes.data, len(order), t.ctypes.data, len(t)) == -EINVAL
        assert lib.rxg_flow_trains_attach(eng.ctx, None, 1, trains.ctypes.data, 1) == -EINVAL
        assert lib.rxg_flow_trains_attach(eng.ctx, order.ctypes.data, 1, None, 1) == -EINVAL
        assert lib.rxg_flow_trains_attach(None, order.ctypes.data, 1, trains.ctypes.data, 1) == -EINVAL
        assert lib.rxg_flow_trains_attach(eng.ctx, None, 0, None, 0) == 0
    finally:
        free(o)
        b.close()


def rxg_stats(eng):
    out = (C.c_uint64 * 4)()
    assert rxg.load_library().rxg_replay_stats(eng.ctx, out) == 0
    return list(out)
