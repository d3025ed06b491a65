"""GPU: rxg_ack_plan_dev (a burst's ACKs planned per flow on the device) against the numpy model
tests/ackplan_ref.py -- never against the kernels' own output or the host function -- on every set
of tests/ackplan_cases.py, on the default grid and on max_blocks 1 and 2 with identical bytes; two
calls on two streams of one context; the whole chain burst -> flow trains -> received options ->
ACK plan -> option build on a real burst of 6 000 frames, the built ACKs received again by the
peer; and rxg_acks_attach / rxg_ack_take around a replay.  segs, acks, opts and the words around
count are pre-filled with 0xA5 and compared whole.  The state table is poisoned past ntcb."""
import ctypes as C

import numpy as np
import pytest
import torch

import ackplan_cases as cases
import ackplan_ref as ref
import flowtrain_ref
import oracle
import pktgen
import rxg
import rxopt_ref
import txbuild_opt_ref as oref
from test_gpu_flowtrain import replay_case, run_replay
from test_gpu_txbuild import _peer_tcbs

pytestmark = pytest.mark.gpu

FILL, FILL64, EINVAL = cases.FILL, 0xA5A5A5A5A5A5A5A5, 22
SETS = cases.all_sets()


class Dev:
    """Set s on the device, with the buffers of one call."""

    def __init__(self, eng, s):
        self.eng, self.s = eng, s
        a = s.args
        self.dev = []
        self.dord, self.dtr = self.up(s.order[:a["cap_seg"]]), self.up(s.trains[:a["cap_trains"]])
        self.dcnt, self.dst = self.up(s.train_count), self.up(s.state)          # (the state with its poison past ntcb)
        self.drx = self.up(s.rxopts) if s.rxopts is not None and len(s.rxopts) else None
        self.want, _ = cases.expect(s)

    def up(self, a):
        a = np.ascontiguousarray(a).view(np.uint8)
        d = self.eng.to_device(a if len(a) else np.zeros(16, np.uint8))
        self.dev.append(d)
        return d

    def outs(self):
        wsegs, wacks, wopts, _ = self.want
        return [self.eng.to_device(np.full(wsegs.nbytes, FILL, np.uint8)), self.eng.to_device(np.full(wacks.nbytes, FILL, np.uint8)),
                self.eng.to_device(self.s.opts_in().view(np.uint8)), self.eng.to_device(np.full(48, FILL, np.uint8))]

    def call(self, eng, o, stream=None):
        s, a = self.s, self.s.args
        eng.ack_plan_dev(self.dord.ptr if a["cap_seg"] else None, a["cap_seg"], self.dtr.ptr if a["cap_trains"] else None,
                         a["cap_trains"], self.dcnt.ptr, s.n, s.ntcb, self.dst.ptr, o[0].ptr, o[1].ptr, a["cap"], o[3].ptr + 8,
                         rxopts=self.drx.ptr if self.drx else None, tsval_now=a["tsval_now"], ip_id0=a["ip_id0"],
                         opt_plain=a["opt_plain"], opt_base=a["opt_base"], opt_cap=a["opt_cap"],
                         opts=o[2].ptr if s.use_opts else None, stream=stream)

    def check(self, o, what=""):
        wsegs, wacks, wopts, wcount = self.want
        what = f"{self.s.name} {what}"
        cw = o[3].download(np.uint64, 6)
        assert cw[[0, 5]].tolist() == [FILL64, FILL64] and cw[1:5].tolist() == wcount.tolist(), (what, cw, wcount)
        segs, acks = o[0].download(np.uint8, wsegs.nbytes), o[1].download(np.uint8, wacks.nbytes)
        opts = o[2].download(np.uint8, wopts.nbytes)
        for got, want, name, size in ((segs, wsegs, "segs", 32), (acks, wacks, "acks", 16), (opts, wopts, "opts", 48)):
            if got.tobytes() != want.tobytes():
                bad = np.nonzero(got != want.view(np.uint8))[0]
                raise AssertionError(f"{what}: {name} differ in {len(bad)} bytes, first in entry {bad[0] // size} at byte "
                                     f"{bad[0] % size}: got {got[bad[0]]} want {want.view(np.uint8)[bad[0]]}")
        return segs.tobytes() + acks.tobytes() + opts.tobytes() + cw.tobytes()

    def run(self, eng=None, what=""):
        eng = eng or self.eng
        o = self.outs()
        try:
            self.call(eng, o)
            eng.sync()
            return self.check(o, what)
        finally:
            free(o)

    def close(self):
        for d in self.dev:
            d.free()


def free(o):
    for d in o:
        d.free()


@pytest.fixture(scope="module")
def capped():
    engs = [rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)]
    yield engs
    for e in engs:
        e.close()


# ----------------------------------------------------- 1. every set on three grids ---
@pytest.mark.parametrize("s", SETS, ids=[s.name for s in SETS])
def test_sets_on_the_default_and_capped_grids(engine, capped, s):
    got = []
    for eng, what in ((engine, "default grid"), (capped[0], "max_blocks 1"), (capped[1], "max_blocks 2")):
        d = Dev(eng, s)
        try:
            got.append(d.run(what=what))
        finally:
            d.close()
    assert got[0] == got[1] == got[2]


# ------------------------------------------------ 2. two streams, no state between ---
def test_two_calls_on_two_streams_of_one_context(engine):
    by = {s.name: s for s in SETS}
    st = torch.cuda.Stream()
    big, small = Dev(engine, by[f"T={cases.ROUND + 1} mixed"]), Dev(engine, by["combos rxopts TS"])
    try:
        outs = [x.outs() for x in (big, small, big, small)]
        big.call(engine, outs[0])
        small.call(engine, outs[1], stream=st.cuda_stream)
        big.call(engine, outs[2], stream=st.cuda_stream)
        small.call(engine, outs[3])
        engine.sync()
        engine.stream_sync(st.cuda_stream)
        for x, o, what in zip((big, small, big, small), outs, ("first", "caller stream", "again", "last")):
            x.check(o, what)
        for o in outs:
            free(o)
    finally:
        big.close()
        small.close()


def test_argument_errors_write_nothing(engine):
    lib = rxg.load_library()
    s = cases.wrap_set()
    d = Dev(engine, s)
    o = d.outs()
    try:
        a = s.args
        good = dict(order=d.dord.ptr, cap_seg=a["cap_seg"], trains=d.dtr.ptr, cap_trains=a["cap_trains"], train_count=d.dcnt.ptr,
                    n=s.n, ntcb=s.ntcb, rxopts=None, state=d.dst.ptr, flags=0, tsval_now=1, ip_id0=2, pad0=0,
                    opt_plain=a["opt_plain"], opt_base=a["opt_base"], opt_cap=a["opt_cap"], opts=o[2].ptr, segs=o[0].ptr,
                    acks=o[1].ptr, cap=a["cap"], count=o[3].ptr + 8)
        bad = [dict(train_count=None), dict(state=None), dict(count=None), dict(order=None), dict(trains=None),
               dict(segs=None), dict(acks=None), dict(opt_plain=3), dict(opt_base=99), dict(ntcb=0),
               dict(ntcb=rxg.FS_MAX_NTCB + 1), dict(flags=1), dict(state=d.dst.ptr + 8), dict(opts=o[2].ptr + 8),
               dict(segs=o[0].ptr + 8), dict(acks=o[1].ptr + 8), dict(rxopts=d.dst.ptr + 8), dict(trains=d.dtr.ptr + 4),
               dict(train_count=d.dcnt.ptr + 4), dict(count=o[3].ptr + 4), dict(order=d.dord.ptr + 2)]
        for over in bad:
            assert lib.rxg_ack_plan_dev(engine.ctx, C.byref(rxg.DevAckPlan(**{**good, **over})), None) == -EINVAL, over
        assert lib.rxg_ack_plan_dev(None, C.byref(rxg.DevAckPlan(**good)), None) == -EINVAL
        assert lib.rxg_ack_plan_dev(engine.ctx, None, None) == -EINVAL
        engine.sync()
        for x in o:
            raw = x.download(np.uint8, x.nbytes)
            assert raw.tobytes() == (s.opts_in().tobytes() if x is o[2] else bytes([FILL]) * len(raw))
    finally:
        free(o)
        d.close()


# ------------------------------------------------------- 3. the chain on a real burst ---
def chain_burst(seed=17, n=6000, nflows=60):
    """Established flows 1 .. nflows (slot 0 a listener), data segments that mostly continue, every
    third flow with timestamps on its segments, some FINs, some pure ACKs, some strangers."""
    rng = np.random.default_rng(seed)
    dst = pktgen.ip4(192, 168, 78, 2)
    rows = [(80, 0, pktgen.raw_of_host(dst), 0, 1)]
    for f in range(nflows):
        rows.append((80, 3000 + f, pktgen.raw_of_host(dst), pktgen.ip4(10, 2, 0, f + 1), 4))
    nxt, first, frames = {}, {}, []
    for i in range(n):
        f = int(rng.integers(0, nflows + 3))
        if f >= nflows:                                            # a stranger: no TCB
            frames.append(pktgen.frame(src_ip=pktgen.ip4(172, 16, 1, f), dst_ip=dst, sport=5000, dport=80, seq=i, flags=0x10,
                                       payload=b"x" * 5))
            continue
        dl = 0 if rng.random() < 0.1 else int(rng.integers(1, 400))
        seq = nxt[f] if f in nxt and rng.random() < 0.9 else int(rng.integers(1, 1 << 32))
        first.setdefault(f, seq) if dl else None
        fin = dl and rng.random() < 0.05
        ts = f % 3 == 0
        opts = bytes([1, 1, 8, 10]) + (100000 + i).to_bytes(4, "big") + (7).to_bytes(4, "big") if ts else None
        frames.append(pktgen.frame(src_ip=pktgen.ip4(10, 2, 0, f + 1), dst_ip=dst, sport=3000 + f, dport=80, seq=seq,
                                   ack=99, flags=0x11 if fin else 0x10, payload=bytes(rng.integers(0, 256, dl, dtype=np.uint8)),
                                   doff=8 if ts else 5, tcp_opts=opts))
        if dl:
            nxt[f] = (seq + dl + (1 if fin else 0)) & 0xFFFFFFFF
    ntcb = len(rows)
    cur = np.zeros(ntcb, np.uint32)
    for f, q in first.items():
        cur[f + 1] = q if f % 2 == 0 else (q - 9) & 0xFFFFFFFF    # odd flows: a gap, their ACK is a duplicate
    st = cases.states(ntcb, seed)
    st["flags"] = rxg.AS_LIVE | np.where((np.arange(ntcb) - 1) % 3 == 0, rxg.AS_TS, 0)
    st["flags"][5] = 0                                             # one flow the stack does not ACK for
    st["rcv_ack"] = cur
    st["ts_recent"] = 50 + np.arange(ntcb)                       # (below every TSval of the burst)
    return rows, frames, cur, st


def test_chain_from_frames_to_ack_frames(engine):
    rows, frames, cur, st = chain_burst()
    n, ntcb = len(frames), len(rows)
    arena, off, lens = pktgen.pack_arena(frames)
    tcb, live = pktgen.table_arrays(rows)
    recs = np.ascontiguousarray(oracle.rx_batch(arena, off, lens, tcb, live)[0]["c"])
    worder, wtrains, wcount = flowtrain_ref.trains(recs.view(np.uint8), rxg.REC16, ntcb, frames, 0, cur)
    wrx = rxopt_ref.records(frames, recs["verdict"])
    opt_base, tsval_now = 1, 0x0BADF00D
    nflows_max = ntcb
    wsegs, wacks, wcnt, blocks = ref.plan(worder, wtrains, wcount, n, ntcb, st, wrx, tsval_now, 0xFFE0, 1, opt_base,
                                          opt_base + nflows_max, True, nflows_max)
    A = int(wcnt[0])
    fl = wacks["flags_train"] & 0xFF
    assert A > 40 and wcnt[1] == 1 and (fl & rxg.ACK_ADVANCES).sum() > 10 and (fl & rxg.ACK_DUP).sum() > 10
    assert (fl & rxg.ACK_FIN).any() and len(blocks) > 10 and int(wtrains["nseg"].max()) > 3
    echoed = [int.from_bytes(bytes(b["bytes"][8:12]), "big") for b in blocks.values()]
    assert sum(e >= 100000 for e in echoed) > 5 and sum(e < 100000 for e in echoed) > 2      # echoes of the burst and ts_recent
    wopts = np.full((opt_base + nflows_max) * 48, FILL, np.uint8).view(rxg.TX_OPT_DTYPE)
    wopts[0] = rxg.tx_opt_ref_ack()[0]
    for k, b in blocks.items():
        wopts[k] = b
    flows = np.zeros(ntcb, dtype=rxg.TX_FLOW_DTYPE)
    for i, r in enumerate(rows):
        flows[i] = (r[0], r[1], r[2], r[3], [2, 0, 10, 2, 0, i & 255], list(rxg.REF_SRC_MAC), [0] * 8)
    aoff = (np.arange(A) * 2).astype(np.uint32)
    wpool, wlens, wstats = oref.build(np.zeros(16, np.uint8), flows, wsegs, wopts, aoff, 2 * A, fill=FILL)
    assert wstats.tolist() == [A, 0]

    eng = engine
    eng.tcb_load(tcb, live)
    up = lambda a: eng.to_device(np.ascontiguousarray(a).view(np.uint8))
    da, do, dl, dcur, dst, dflows = up(arena), up(off), up(lens), up(cur), up(st), up(flows)
    drec, dord, dtr = eng.alloc(n * 16), eng.alloc(n * 4), eng.alloc(n * 32)
    dcnt, drx = eng.alloc(32), eng.alloc(n * 16)
    dsegs, dacks = up(np.full(nflows_max * 32, FILL, np.uint8)), up(np.full(nflows_max * 16, FILL, np.uint8))
    o0 = np.full(wopts.nbytes, FILL, np.uint8)
    o0[:48] = wopts[:1].view(np.uint8)
    dopts, dc, dpay = up(o0), up(np.full(48, FILL, np.uint8)), up(np.zeros(16, np.uint8))
    dpool, dlen, dstats = up(np.full(2 * A * 64, FILL, np.uint8)), up(np.zeros(A, np.uint16)), up(np.zeros(2, np.uint64))
    daoff = up(aoff)
    every = [da, do, dl, dcur, dst, dflows, drec, dord, dtr, dcnt, drx, dsegs, dacks, dopts, dc, dpay, dpool, dlen, dstats, daoff]
    try:
        eng.rx_burst_dev(da.ptr, do.ptr, dl.ptr, n, drec.ptr, rxg.REC16)
        eng.flow_trains_dev(drec.ptr, rxg.REC16, n, ntcb, dord.ptr, n, dtr.ptr, n, dcnt.ptr, cur_seq=dcur.ptr, frames=da.ptr,
                            lens=dl.ptr, off64=do.ptr)
        eng.rx_opts_dev(da.ptr, dl.ptr, n, drec.ptr, rxg.REC16, drx.ptr, off64=do.ptr)
        eng.ack_plan_dev(dord.ptr, n, dtr.ptr, n, dcnt.ptr, n, ntcb, dst.ptr, dsegs.ptr, dacks.ptr, nflows_max, dc.ptr + 8,
                         rxopts=drx.ptr, tsval_now=tsval_now, ip_id0=0xFFE0, opt_plain=1, opt_base=opt_base,
                         opt_cap=opt_base + nflows_max, opts=dopts.ptr)
        # the host reads only the count: how many frames to build
        eng.sync()
        cw = dc.download(np.uint64, 6)
        assert cw.tolist() == [FILL64] + wcnt.tolist() + [FILL64]
        eng.tx_build_opt_dev(dpay.ptr, 16, dflows.ptr, ntcb, dsegs.ptr, A, dpool.ptr, dlen.ptr, dopts.ptr, opt_base + nflows_max,
                             off64=daoff.ptr, stats=dstats.ptr)
        eng.sync()
        assert drec.download(rxg.REC16_DTYPE, n).tobytes() == recs.tobytes()
        assert dsegs.download(np.uint8, nflows_max * 32)[:A * 32].tobytes() == wsegs.tobytes()
        assert (dsegs.download(np.uint8, nflows_max * 32)[A * 32:] == FILL).all()
        assert dacks.download(np.uint8, nflows_max * 16)[:A * 16].tobytes() == wacks.tobytes()
        assert dopts.download(np.uint8, wopts.nbytes).tobytes() == wopts.tobytes()
        pool, blen = dpool.download(np.uint8, 2 * A * 64), dlen.download(np.uint16, A)
        assert dstats.download(np.uint64, 2).tolist() == [A, 0] and blen.tolist() == wlens.tolist()
        assert pool.tobytes() == wpool.tobytes()
        with rxg.Engine(device=0) as peer:
            peer.tcb_load(_peer_tcbs(flows), np.ones(ntcb, np.uint8))
            back = peer.rx_arena(pool, aoff, blen, rxg.REC48)
        assert (back["c"]["verdict"] == rxg.V_DISPATCH).all()
        assert (back["c"]["ip_cksum"] == 0).all() and (back["c"]["tcp_cksum"] == 0).all()
        assert back["c"]["tcb_idx"].tolist() == wsegs["flow"].tolist() and (back["c"]["datalen"] == 0).all()
        assert back["seq"].tolist() == wsegs["seq"].tolist() and back["ack"].tolist() == wsegs["ack"].tolist()
    finally:
        free(every)


# --------------------------------------------------------------------- 4. the replay ---
def test_take_around_a_replay(replay_engine):
    eng = replay_engine
    lib = rxg.load_library()
    rc = replay_case()
    rows, frames, recs16, erows, exp = (rc[k] for k in ("rows", "frames", "recs16", "erows", "exp"))
    n, ntcb = len(frames), len(rows)
    st = cases.states(ntcb, 3)
    st["flags"] = rxg.AS_LIVE
    wcount = np.array([len(rc["worder"]), len(rc["wtrains"]), 0, 0], np.uint64)
    wsegs, wacks, wcnt, _ = ref.plan(rc["worder"], rc["wtrains"], wcount, n, ntcb, st)
    A = int(wcnt[0])
    changed_tcb = set()
    for i in rc["changed"]:
        changed_tcb |= {int(recs16["tcb_idx"][i]), exp[i][1]}
    written = {i for i in range(ntcb) if rows[i] != erows[i]}
    void = changed_tcb | written
    flows_acked = set(wacks["tcb_idx"].tolist())
    assert len(flows_acked & changed_tcb) > 0 and len(flows_acked & written) > 0 and len(flows_acked - void) > 5
    eng.tcb_load(*pktgen.table_arrays(rows))
    arena, off, lens = pktgen.pack_arena(frames)
    up = lambda a: eng.to_device(np.ascontiguousarray(a).view(np.uint8))
    da, do, dl, dr = up(arena), up(off), up(lens), eng.alloc(n * 16)
    dord, dtr, dcnt, dst = up(rc["worder"]), up(rc["wtrains"]), up(wcount), up(st)
    dsegs, dacks, dc = eng.alloc(max(A, 1) * 32), eng.alloc(max(A, 1) * 16), eng.alloc(32)
    try:
        eng.rx_burst_dev(da.ptr, do.ptr, dl.ptr, n, dr.ptr, rxg.REC16)           # the burst the replay replays
        eng.ack_plan_dev(dord.ptr, len(rc["worder"]), dtr.ptr, len(rc["wtrains"]), dcnt.ptr, n, ntcb, dst.ptr, dsegs.ptr,
                         dacks.ptr, A, dc.ptr)
        eng.sync()
        acks = dacks.download(rxg.ACK_DTYPE, A).copy()
        assert acks.tobytes() == wacks.tobytes() and dc.download(np.uint64, 4).tolist() == wcnt.tolist()
        recs = dr.download(rxg.REC16_DTYPE, n)
        assert recs.tobytes() == recs16.tobytes()
        built = np.zeros(A * 64, np.uint8)                                        # (the frames' bytes: section 3)
        base = built.ctypes.data
        clean = sorted(flows_acked - void)
        where = {int(t): k for k, t in enumerate(acks["tcb_idx"].tolist())}
        take = lambda t, ds=0, da_=0: eng.ack_take(t, int(acks[where[t]]["seq"]) + ds, int(acks[where[t]]["ack"]) + da_)
        assert eng.ack_take(clean[0], 0, 0) is None                              # nothing attached
        eng.acks_attach(acks.ctypes.data, base, 64, A)
        assert take(clean[0]) is None                                             # attached, but its replay has not begun
        during = []
        run_replay(eng, rows, frames, recs, lambda i: during.append(take(clean[0])))
        assert during and all(x == base + 64 * where[clean[0]] for x in during)  # inside the handlers
        # after the replay returned: untouched flows 1, everything the replay touched 0
        for t in sorted(flows_acked):
            got = take(t)
            if t in void:
                assert got is None, (t, t in changed_tcb, t in written)
            else:
                assert got == base + 64 * where[t], t
        t = clean[1]
        assert take(t, da_=1) is None and take(t, ds=1) is None and take(t) is not None     # the stack's own state decides
        assert eng.ack_take(ntcb + 5, 0, 0) is None and eng.ack_take(-1, 0, 0) is None
        p = C.c_void_p()
        assert lib.rxg_ack_take(eng.ctx, t, 0, 0, None) == -EINVAL and lib.rxg_ack_take(None, t, 0, 0, C.byref(p)) == -EINVAL
        # a write to the slot after the replay returned voids its ACK too; other flows keep theirs
        t2 = clean[2]
        assert take(t2) is not None
        eng.tcb_set_state(t2, rows[t2][4])
        assert take(t2) is None and take(t) is not None
        # the next replay ends the attachment
        ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(), rxg.HANDOFF_ADD_MAC(),
                             rxg.HANDOFF_SEND_RESET(), rxg.HANDOFF_ON_SEGMENT(), rxg.HANDOFF_TCPSWITCH())
        assert lib.rxg_rx_replay(eng.ctx, C.byref(ops), None, None, None, 0, 16) == 0
        assert take(t) is None
        # attach: sorted by tcb_idx, no NULLs, a stride
        swapped = acks.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        twice = acks.copy()
        twice["tcb_idx"][1] = twice["tcb_idx"][0]
        for x in (swapped, twice):
            assert lib.rxg_acks_attach(eng.ctx, x.ctypes.data, base, 64, A) == -EINVAL
        assert lib.rxg_acks_attach(eng.ctx, None, base, 64, 1) == -EINVAL
        assert lib.rxg_acks_attach(eng.ctx, acks.ctypes.data, None, 64, 1) == -EINVAL
        assert lib.rxg_acks_attach(eng.ctx, acks.ctypes.data, base, 0, 1) == -EINVAL
        assert lib.rxg_acks_attach(None, acks.ctypes.data, base, 64, 1) == -EINVAL
        assert lib.rxg_acks_attach(eng.ctx, None, None, 0, 0) == 0
        # a replay that fails its argument checks ends the attachment: nothing of a burst that was
        # not replayed is handed out, by that call or by a later one
        eng.acks_attach(acks.ctypes.data, base, 64, A)
        assert lib.rxg_rx_replay(eng.ctx, None, None, None, None, 0, 16) == -EINVAL
        assert take(t) is None
        assert lib.rxg_rx_replay(eng.ctx, C.byref(ops), None, None, None, 0, 16) == 0
        assert take(t) is None
        # a second attach replaces the first before its replay
        eng.acks_attach(acks.ctypes.data, base, 64, A)
        eng.acks_attach(acks.ctypes.data, base, 64, 0)
        assert lib.rxg_rx_replay(eng.ctx, C.byref(ops), None, None, None, 0, 16) == 0
        assert take(t) is None
    finally:
        free([da, do, dl, dr, dord, dtr, dcnt, dst, dsegs, dacks, dc])
