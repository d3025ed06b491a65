"""GPU: rxg_train_payload_dev (a burst's payload gathered by train on the device) against the
numpy model tests/trainpay_ref.py -- never against the kernels' own output or the host function
-- on every set of tests/trainpay_cases.py (its claims are asserted in
tests/test_trainpay_host.py), for 8-, 16- and 48-byte records, frames through off64 and through a
stride, on the default grid and on max_blocks 1 and 2.  Narrower than that in two places, for run
time: the three scan-round sets (65 535 to 65 537 frames) run in one record kind each through
off64 only -- the offset scan reads neither records nor frames -- and set 9, whose 65 535-byte
frame would make a fixed stride of 1 024 slots, runs through off64 only.  The arena, msgs, tmsgs
and the words around arena_used are pre-filled with 0xA5 and compared whole.  Then the multiflow
exchange of tests/test_gpu_payload.py with this call in place of the gather: the socket-ring
messages equal the reference's."""
import ctypes as C

import numpy as np
import pytest

import c1_stack as c1
import pktgen
import rxg
import trainpay_cases as cases
import trainpay_ref as ref
from test_gpu_payload import multiflow_bursts

pytestmark = pytest.mark.gpu

FILL, EINVAL, SLACK = 0xA5, 22, 64
FILL64 = 0xA5A5A5A5A5A5A5A5
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
SETS = cases.all_sets()
BIG = 5000          # sets above this many frames run in one record kind only


class Dev:
    """Burst b on the device in one record kind, with the flow-train model's outputs for it."""

    def __init__(self, eng, b, kind, strided=False):
        self.eng, self.b, self.kind = eng, b, kind
        self.order, self.trains, self.count = b.trains(kind)
        self.geom = b.strided() if strided else None
        self.pool = self.geom[0] if self.geom else b.pool
        self.off64 = (self.geom[1] + np.arange(b.n) * self.geom[2]).astype(np.uint32) if self.geom else b.off64
        self.dev = []
        self.dp, self.dl, self.dr = self.up(self.pool), self.up(b.lens), self.up(b.records(kind))
        self.do = None if self.geom else self.up(b.off64)
        self.dord, self.dtr, self.dcnt = self.up(self.order), self.up(self.trains), self.up(self.count)

    def up(self, a):
        a = np.ascontiguousarray(a).view(np.uint8)
        d = self.eng.to_device(a if len(a) else np.zeros(16, np.uint8))
        self.dev.append(d)
        return d

    def want(self, **kw):
        return cases.model(self.b, self.kind, pool=self.pool, off64=self.off64, **kw)

    def outs(self, given, msgs=True, tmsgs=True):
        order, trains, count, cap_seg, cap_trains, arena_cap = given
        full = int(ref.pad16(trains["bytes"].astype(np.int64)).sum())
        return dict(arena=self.eng.to_device(np.full(min(arena_cap, full) + SLACK, FILL, np.uint8)),
                    msgs=self.eng.to_device(np.full(max(self.b.n, 1) * 16, FILL, np.uint8)),
                    tmsgs=self.eng.to_device(np.full((cap_trains + 4) * 16, FILL, np.uint8)),
                    used=self.eng.to_device(np.full(24, FILL, np.uint8)), given=given, use=(msgs, tmsgs))

    def args(self, o, flags=0, **over):
        order, trains, count, cap_seg, cap_trains, arena_cap = o["given"]
        a = dict(frames=self.dp.ptr, off64=None if self.geom else self.do.ptr, len=self.dl.ptr,
                 slot0=self.geom[1] if self.geom else 0, stride64=self.geom[2] if self.geom else 0, n=self.b.n,
                 rec_kind=self.kind, recs=self.dr.ptr, order=self.dord.ptr if cap_seg else None, cap_seg=cap_seg,
                 trains=self.dtr.ptr if cap_trains else None, cap_trains=cap_trains, count=self.dcnt.ptr, flags=flags,
                 arena=o["arena"].ptr, arena_cap=arena_cap, msgs=o["msgs"].ptr if o["use"][0] else None,
                 tmsgs=o["tmsgs"].ptr if o["use"][1] else None, arena_used=o["used"].ptr + 8)
        a.update(over)
        return rxg.DevTrainPayload(**a)

    def call(self, eng, o, flags=0, stream=None):
        lib = rxg.load_library()
        rc = lib.rxg_train_payload_dev(eng.ctx, C.byref(self.args(o, flags)), stream)
        assert rc == 0, lib.rxg_last_error()

    def check(self, o, want, what):
        warena, wm, wtm, wused = want
        msgs, tmsgs = o["use"]
        used = o["used"].download(np.uint64, 3)
        assert used.tolist() == [FILL64, wused, FILL64], (what, used, wused)
        arena = o["arena"].download(np.uint8, len(warena))
        if arena.tobytes() != warena.tobytes():
            bad = np.nonzero(arena != warena)[0]
            raise AssertionError(f"{what}: {len(bad)} arena bytes differ, first at {bad[0]}: got {arena[bad[0]]} want "
                                 f"{warena[bad[0]]}")
        m = o["msgs"].download(np.uint8, max(self.b.n, 1) * 16)
        if msgs:
            m = m.view(rxg.PAYLOAD_MSG_DTYPE)[:self.b.n]
            assert m.tobytes() == wm.tobytes(), (what, "msgs", np.nonzero(m != wm)[0][:5])
        else:
            assert (m == FILL).all(), (what, "msgs written though NULL was given")
        cap_trains = o["given"][4]
        tm = o["tmsgs"].download(np.uint8, (cap_trains + 4) * 16).view(rxg.PAYLOAD_MSG_DTYPE)
        t = len(wtm) if tmsgs else 0
        if tmsgs:
            assert tm[:t].tobytes() == wtm.tobytes(), (what, "tmsgs", np.nonzero(tm[:t] != wtm)[0][:5])
        assert (tm[t:].view(np.uint8) == FILL).all(), (what, "tmsgs written at or past T'")
        return arena.tobytes() + m.tobytes() + tm.tobytes() + used.tobytes()

    def run(self, eng=None, what="", flags=0, want_msgs=True, want_tmsgs=True, **kw):
        eng = eng or self.eng
        want, given = self.want(flags=flags, want_msgs=want_msgs, want_tmsgs=want_tmsgs, **kw)
        o = self.outs(given, want_msgs, want_tmsgs)
        try:
            self.call(eng, o, flags)
            eng.sync()
            return self.check(o, want, f"{self.b.name}, records of {self.kind} {what}"), want
        finally:
            free(o)

    def close(self):
        for d in self.dev:
            d.free()


def free(o):
    for k in ("arena", "msgs", "tmsgs", "used"):
        o[k].free()


@pytest.fixture(scope="module")
def capped():
    engs = [rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)]
    yield engs
    for e in engs:
        e.close()


# ------------------------------- 1. every set, every layout, both pools, three grids ---
@pytest.mark.parametrize("b", SETS, ids=[b.name for b in SETS])
def test_sets_in_every_layout_and_on_capped_grids(engine, capped, b):
    small = b.n <= BIG
    pools = [False, True] if small and b.strided() is not None else [False]
    assert not small or b.name.startswith("9") or len(pools) == 2             # the strided pool is used
    for kind in (KINDS if small else [KINDS[b.n % 3]]):
        for strided in pools:
            d = Dev(engine, b, kind, strided=strided)
            try:
                what = "strided, " if strided else "off64, "
                a, _ = d.run(what=what + "default grid")
                assert a == d.run(capped[0], what=what + "max_blocks 1")[0]
                assert a == d.run(capped[1], what=what + "max_blocks 2")[0]
            finally:
                d.close()


# ----------------------------------------------------------------- 2. caps and flags ---
def test_caps_flags_null_outputs_and_no_state_between_calls(engine):
    import torch
    b = cases.by_name("7:")
    for kind in KINDS:
        d = Dev(engine, b, kind)
        try:
            _, (warena, wm, wtm, used) = d.run()
            trains = d.trains
            ends = (wtm["arena_off"] + ref.pad16(trains["bytes"].astype(np.int64)).astype(np.uint64)).tolist()
            for cap in (0, ends[3] - 1, ends[3], ends[3] + 1, 15, (1 << 64) - 1, 1 << 32, (1 << 32) + ends[3] - 1, 1 << 63):
                _, w = d.run(what=f"arena_cap {cap}", arena_cap=cap)
                assert w[3] == used and int(((w[2]["flags"] & rxg.PM_GATHERED) != 0).sum()) == sum(e <= cap for e in ends)
            d.run(what="cap_seg inside a train", cap_seg=int(trains[2]["first"]) + 1)
            d.run(what="cap_trains short of T", cap_trains=4)
            _, w = d.run(what="HEAD only", flags=rxg.TP_HEAD_ONLY)
            assert [int(f) != 0 for f in w[2]["flags"]] == [True, False, True, False, False, True]
            d.run(what="msgs NULL", want_msgs=False)
            d.run(what="tmsgs NULL", want_tmsgs=False)
            _, w = d.run(what="cap_seg 0", cap_seg=0)
            assert w[3] == 0 and len(w[2]) == 0
            d.run(what="cap_trains 0", cap_trains=0)
        finally:
            d.close()
    # two different bursts back to back on one context, no host wait, another stream in between
    s = torch.cuda.Stream()
    big, small = Dev(engine, cases.by_name("3: trains"), rxg.REC16), Dev(engine, cases.by_name("2:"), rxg.REC8)
    try:
        wants = [big.want(), small.want(), big.want(), small.want()]
        outs = [x.outs(w[1]) for x, w in zip((big, small, big, small), wants)]
        big.call(engine, outs[0])
        small.call(engine, outs[1], stream=s.cuda_stream)
        big.call(engine, outs[2], stream=s.cuda_stream)
        small.call(engine, outs[3])
        engine.sync()
        engine.stream_sync(s.cuda_stream)
        for x, o, w, what in zip((big, small, big, small), outs, wants, ("first", "caller stream", "again", "last")):
            x.check(o, w[0], what)
        for o in outs:
            free(o)
    finally:
        big.close()
        small.close()


# ----------------------------------------------------- 3. n == 0 and argument errors ---
def test_argument_errors_and_empty_bursts_write_nothing(engine):
    lib = rxg.load_library()
    b = cases.by_name("2:")
    d = Dev(engine, b, rxg.REC16)
    s = Dev(engine, b, rxg.REC16, strided=True)
    want, given = d.want()
    o = d.outs(given)
    try:
        bad = [(dict(frames=None), b"NULL"), (dict(len=None), b"NULL"), (dict(recs=None), b"NULL"),
               (dict(order=None), b"NULL"), (dict(trains=None), b"NULL"), (dict(count=None), b"NULL"),
               (dict(arena_used=None), b"NULL"), (dict(arena=None), b"NULL"),
               (dict(rec_kind=0), b"rec_kind"), (dict(rec_kind=32), b"rec_kind"),
               (dict(flags=2), b"flags"), (dict(flags=0x80000001), b"flags"),
               (dict(frames=d.dp.ptr + 8), b"alignment"), (dict(arena=o["arena"].ptr + 8), b"alignment"),
               (dict(msgs=o["msgs"].ptr + 4), b"alignment"), (dict(tmsgs=o["tmsgs"].ptr + 4), b"alignment"),
               (dict(trains=d.dtr.ptr + 4), b"alignment"), (dict(count=d.dcnt.ptr + 4), b"alignment"),
               (dict(arena_used=o["used"].ptr + 12), b"alignment"), (dict(order=d.dord.ptr + 2), b"alignment"),
               (dict(off64=d.do.ptr + 2), b"alignment"), (dict(len=d.dl.ptr + 1), b"alignment"),
               (dict(recs=d.dr.ptr + 8), b"alignment"), (dict(recs=d.dr.ptr + 4, rec_kind=rxg.REC8), b"alignment"),
               (dict(off64=None, stride64=0), b"stride64"),
               (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
               (dict(off64=None, slot0=0, stride64=0xFFFFFFFF, n=3), b"2^32")]
        for kw, why in bad:
            assert lib.rxg_train_payload_dev(engine.ctx, C.byref(d.args(o, **kw)), None) == -EINVAL, kw
            assert why in lib.rxg_last_error(), (kw, lib.rxg_last_error())
        assert lib.rxg_train_payload_dev(engine.ctx, None, None) == -EINVAL
        assert lib.rxg_train_payload_dev(None, C.byref(d.args(o)), None) == -EINVAL
        engine.sync()

        def untouched(*names):
            return all((o[k].download(np.uint8, o[k].nbytes) == FILL).all() for k in names)
        assert untouched("arena", "msgs", "tmsgs", "used")
        # n == 0: arena_used = 0 and nothing else, in either addressing mode
        for x, kw in ((d, dict(n=0)), (s, dict(n=0)), (d, dict(n=0, msgs=None, tmsgs=None, arena=None, arena_cap=0))):
            assert lib.rxg_train_payload_dev(engine.ctx, C.byref(x.args(o, **kw)), None) == 0, lib.rxg_last_error()
            engine.sync()
            assert o["used"].download(np.uint64, 3).tolist() == [FILL64, 0, FILL64]
            assert untouched("arena", "msgs", "tmsgs")
            o["used"].upload(np.full(24, FILL, np.uint8))
        # and the valid call works
        d.call(engine, o)
        engine.sync()
        d.check(o, want, "the valid call")
    finally:
        free(o)
        d.close()
        s.close()
    # S == 0: a burst without segments -- used = 0, msgs zeroed, nothing else
    none = cases.build("no segments", cases.ftc.craft([1, 1], [5, 6], [0, 0]), 2)
    d = Dev(engine, none, rxg.REC16)
    try:
        _, w = d.run(what="S == 0")
        assert w[3] == 0 and not w[1].view(np.uint8).any()
    finally:
        d.close()


# --------------------------------------------------------------------- 4. the replay ---
def drive_trains(engine, bursts):
    """c1_stack.drive_rxg with the payload gathered by train: per burst rxg_rx_burst_dev,
    rxg_flow_trains_dev, rxg_train_payload_dev, then the replay whose PushData takes the
    messages through rxg_payload_take."""
    st = c1.Stack()
    st.sent = []
    st.mirror = engine
    engine.tcb_load(*pktgen.table_arrays(st.rows))
    engine.arp_disable()
    lib = rxg.load_library()
    ntcb, holes = 4096, 0
    for burst in bursts:
        frames = [c1.with_checksums(f) for f in burst]
        n = len(frames)
        arena, off, lens = pktgen.pack_arena(frames)
        cap = 4096 + 2048 * n
        dev = [engine.to_device(arena), engine.to_device(off.view(np.uint8)), engine.to_device(lens.view(np.uint8)),
               engine.alloc(n * 16), engine.alloc(n * 4), engine.alloc(n * 32), engine.alloc(32), engine.alloc(cap),
               engine.alloc(n * 16), engine.alloc(n * 16), engine.alloc(8)]
        da, do, dl, dr, dord, dtr, dcnt, dar, dm, dtm, du = dev
        try:
            engine.rx_burst_dev(da.ptr, do.ptr, dl.ptr, n, dr.ptr, rxg.REC16)
            engine.flow_trains_dev(dr.ptr, rxg.REC16, n, ntcb, dord.ptr, n, dtr.ptr, n, dcnt.ptr, frames=da.ptr,
                                   lens=dl.ptr, off64=do.ptr)
            engine.train_payload_dev(da.ptr, dl.ptr, n, dr.ptr, rxg.REC16, dord.ptr, n, dtr.ptr, n, dcnt.ptr, dar.ptr, cap,
                                     dm.ptr, dtm.ptr, du.ptr, off64=do.ptr)
            engine.sync()
            recs = dr.download(rxg.REC16_DTYPE, n)
            T = int(dcnt.download(np.uint64, 4)[1])
            assert int(du.download(np.uint64, 1)[0]) <= cap
            holes += int(((dtm.download(rxg.PAYLOAD_MSG_DTYPE, n)[:T]["flags"] & rxg.PM_HOLE) != 0).sum())
            st.payload = dar.download(np.uint8, cap)
            bufs = [C.create_string_buffer(f, max(len(f), 64)) for f in frames]
            addr = {C.addressof(x): i for i, x in enumerate(bufs)}

            def tcpswitch(u, idx, state, tcp, ip, m):
                i = addr[m]
                st.tcpswitch(idx, state, frames[i], int(recs[i]["datalen"]))
                return 0

            def rst(u, ip, tcp):
                st.send_reset(frames[addr[ip - 14]])

            ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(),
                                 rxg.HANDOFF_ADD_MAC(), rxg.HANDOFF_SEND_RESET(rst), rxg.HANDOFF_ON_SEGMENT(),
                                 rxg.HANDOFF_TCPSWITCH(tcpswitch))
            ptrs = (C.c_void_p * n)(*[C.addressof(x) for x in bufs])
            assert lib.rxg_rx_replay(engine.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n, 16) == 0
        finally:
            for x in dev:
                x.free()
        if st.tx:
            arena, off, lens = pktgen.pack_arena(st.tx)
            out = engine.tx_arena(arena, off, lens)
            st.sent += [bytes(out[int(o) * 64:int(o) * 64 + int(ln)]) for o, ln in zip(off, lens)]
            st.tx = []
    return st, holes


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_multiflow_exchange_by_train_equals_reference(engine, seed):
    bursts = multiflow_bursts(seed)
    want = c1.drive_cpu(bursts)
    got, holes = drive_trains(engine, bursts)
    assert got.rings == want.rings                   # every socket-ring message, per TCB
    assert got.log == want.log and got.rows == want.rows
    assert {i: t["ack"] for i, t in got.tcb.items()} == {i: t["ack"] for i, t in want.tcb.items()}
    assert got.sent == want.sent
    # the segments of flows the burst's table already held came from the trains' spans
    assert got.taken > 100 and holes == 0
