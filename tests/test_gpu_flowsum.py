"""GPU: rxg_flow_sums_dev (a burst summarised per flow on the device) and the summaries' use during
the replay (rxg_flow_sums_attach / rxg_flow_sum_current) against the numpy model
tests/flowsum_ref.py fed the CPU oracle's records (or the crafted ones) -- never against the
kernel's own output or the host function alone.  Records come from a real rxg_rx_burst_dev where
the case allows.  Outputs are pre-filled with 0xA5 and compared whole, eight guard entries and
the words around `count` included."""
import ctypes as C

import numpy as np
import pytest

import flowsum_cases as cases
import flowsum_ref as ref
import oracle
import pktgen
import rxg
from test_gpu_replay import Model, scenario, sequential_reference

pytestmark = pytest.mark.gpu

FILL, GUARD, EINVAL = 0xA5, 8, 22
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
TILE = rxg.FLOW_SUM_TILE_TCBS          # TCBs per count tile of the touched bitmap
ROUND = rxg.FLOW_SUM_SCAN_TILES        # tiles per round of the scan


class Batch:
    """Records on the device -- crafted (rec48 given) or written by a real burst of `frames` on
    `rows` -- with the model's answer for them."""

    def __init__(self, eng, rec_kind, ntcb, rec48=None, frames=None, rows=None, flags=0, strided=False, no_frames=False):
        self.eng, self.rec_kind, self.ntcb, self.flags = eng, rec_kind, ntcb, flags
        self.dev = []
        real = rec48 is None
        if frames is None and not (no_frames and rec_kind == rxg.REC48):
            frames = cases.frames_for(rec48)
        self.frames, self.geom = frames, None
        self.n = len(frames) if frames is not None else len(rec48)
        self.da = self.do = self.dl = None
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
        if real:
            tcb, live = pktgen.table_arrays(rows)
            eng.tcb_load(tcb, live)
            self.dr = self.up(np.full(self.n * rec_kind, FILL, np.uint8))
            eng.rx_burst_dev(self.da.ptr, self.do.ptr, self.dl.ptr, self.n, self.dr.ptr, rec_kind)
            eng.sync()
            rec48 = oracle.rx_batch(arena, off, lens, tcb, live)[0]
        else:
            self.dr = self.up(cases.as_kind(rec48, rec_kind).view(np.uint8))
        self.rec48 = rec48
        self.want, self.wcount = ref.summaries(cases.as_kind(rec48, rec_kind), rec_kind, ntcb, frames, flags)
        self.m = len(self.want)

    def up(self, a):
        d = self.eng.to_device(np.ascontiguousarray(a).view(np.uint8) if len(a) else np.zeros(16, np.uint8))
        self.dev.append(d)
        return d

    def outs(self, cap=None):
        cap = self.m if cap is None else cap
        return (self.eng.to_device(np.full((cap + GUARD) * 40, FILL, np.uint8)),
                self.eng.to_device(np.full(5 * 8, FILL, np.uint8)), cap)

    def call(self, eng, o, stream=None, use_stride=False):
        out, count, cap = o
        eng.flow_sums_dev(self.dr.ptr, self.rec_kind, self.n, self.ntcb, out.ptr, cap, count.ptr + 8,
                          frames=None if self.da is None else self.da.ptr, lens=None if self.dl is None else self.dl.ptr,
                          off64=None if (use_stride or self.do is None) else self.do.ptr,
                          slot0=self.geom[0] if use_stride else 0, stride64=self.geom[1] if use_stride else 0,
                          flags=self.flags, stream=stream)

    def check(self, o, what=""):
        out, count, cap = o
        cw = count.download(np.uint64, 5)
        assert cw[0] == cw[4] == 0xA5A5A5A5A5A5A5A5, (what, "words around count were written")
        assert cw[1:4].tolist() == self.wcount.tolist(), (what, cw[1:4], self.wcount)
        got = out.download(np.uint8, (cap + GUARD) * 40).view(rxg.FLOW_SUM_DTYPE)
        k = min(self.m, cap)
        if got[:k].tobytes() != self.want[:k].tobytes():
            bad = [i for i in range(k) if got[i] != self.want[i]]
            raise AssertionError(f"{what}: {len(bad)} of {k} summaries differ, first at {bad[0]}: got {got[bad[0]]} "
                                 f"want {self.want[bad[0]]}")
        assert (got[k:].view(np.uint8) == FILL).all(), (what, "entries at or past min(count, cap) were written")
        return got[:k].tobytes() + cw[1:4].tobytes()

    def run(self, eng=None, what="", cap=None, **kw):
        eng = eng or self.eng
        o = self.outs(cap)
        try:
            self.call(eng, o, **kw)
            eng.sync()
            return self.check(o, what)
        finally:
            o[0].free()
            o[1].free()

    def close(self):
        for d in self.dev:
            d.free()


def crafted(eng, tcb, rec_kind=rxg.REC8, ntcb=None, seed=1, **kw):
    """Crafted DISPATCH records on the flows `tcb` with random seq / ack / datalen / flags."""
    tcb = np.asarray(tcb)
    rng = np.random.default_rng(seed)
    n = len(tcb)
    r = cases.craft(tcb, seq=rng.integers(0, 2**32, n), ack=rng.integers(0, 2**32, n), datalen=rng.integers(-3, 1461, n),
                    tcp_flags=rng.choice([0x10, 0x18, 0x11], n))
    for f, v in kw.pop("fields", {}).items():
        c = r["c"]
        c[f] = v
        r["c"] = c
    return Batch(eng, rec_kind, int(tcb.max()) + 1 if ntcb is None else ntcb, rec48=r, **kw)


def run_close(b, **kw):
    try:
        return b.run(**kw)
    finally:
        b.close()


@pytest.fixture(scope="module")
def one_block():
    e = rxg.Engine(device=0, max_blocks=1)
    yield e
    e.close()


# ------------------------------------------------- 1. slice, wave and workgroup edges ---
@pytest.fixture(scope="module")
def real_traffic():
    rng = np.random.default_rng(11)
    flow_of = np.where(rng.random(1025) < 0.1, -1, rng.integers(0, 37, 1025))
    return cases.table(37), cases.traffic(flow_of.tolist(), seed=4, bad_ck=0.05)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_sizes_on_a_real_burst_and_both_grids(engine, one_block, real_traffic, n):
    rows, frames = real_traffic
    b = Batch(engine, rxg.REC8, len(rows), frames=frames[:n], rows=rows)
    try:
        assert n < 64 or (b.m > 5 and int(b.wcount[0]) == b.m)
        assert b.run(what=f"n {n}") == b.run(one_block, what=f"n {n}, max_blocks 1")
    finally:
        b.close()


# ----------------------------------------- 2. the wave-uniform path and its neighbours ---
def uniform_cases():
    one = np.full(64, 9)
    out = {"one flow": one, "64 distinct": np.arange(64)[::-1].copy(), "two alternating": np.tile([3, 8], 32),
           "uniform then another then uniform": np.concatenate([one, np.full(64, 2), one, np.arange(64), one])}
    for lane in (0, 31, 32, 63):
        t = one.copy()
        t[lane] = 4
        out[f"63 of one and another at lane {lane}"] = t
    return out


@pytest.mark.parametrize("name", list(uniform_cases()))
@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC48])
def test_wave_uniform_path_and_neighbours(engine, one_block, name, rec_kind):
    b = crafted(engine, uniform_cases()[name], rec_kind, ntcb=70)
    try:
        assert b.run(what=name) == b.run(one_block, what=name + ", max_blocks 1")
    finally:
        b.close()


def test_uniform_wave_with_other_verdicts_and_an_empty_slice(engine):
    rng = np.random.default_rng(3)
    tcb = np.full(192, 9)
    verdict = np.where(rng.random(192) < 0.5, rxg.V_DISPATCH, rng.integers(1, 6, 192)).astype(np.uint8)
    verdict[64:128] = rng.integers(1, 6, 64)       # a slice without a counted frame
    tcb[np.nonzero(verdict)[0][::3]] = 40          # other verdicts name other flows: ignored
    b = crafted(engine, tcb, ntcb=64, fields={"verdict": verdict})
    assert b.m == 1 and int(b.want[0]["frames"]) == int((verdict == 0).sum()) and b.wcount.tolist() == [1, 0, 0]
    run_close(b, what="partly non-DISPATCH")


# --------------------------------------------------------- 3. bitmap and tile edges ---
def test_bitmap_word_and_tile_edges(engine):
    tcb = np.array([31, 32, 63, 64, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 31, TILE, 0])
    run_close(crafted(engine, tcb, ntcb=2 * TILE + 1), what="word and tile edges")


@pytest.mark.parametrize("ntcb", [33, 95, TILE + 7])
def test_ntcb_not_a_multiple_of_32_and_a_lone_last_flow(engine, ntcb):
    run_close(crafted(engine, np.array([ntcb - 1] * 3), ntcb=ntcb), what="lone flow at ntcb - 1")
    b = crafted(engine, np.array([0, ntcb - 1, ntcb, ntcb + 31, -1, ntcb - 2]), ntcb=ntcb)
    assert b.wcount.tolist() == [3, 3, 0]
    run_close(b, what="around ntcb")


def test_two_scan_rounds_of_tiles(engine, one_block):
    ntcb = (ROUND + 1) * TILE + 5            # ROUND + 2 tiles: the scan takes two rounds
    tcb = np.array([5, TILE - 1, 6, ntcb - 1, ROUND * TILE, ROUND * TILE - 1, (ROUND + 1) * TILE, 5])
    b = crafted(engine, tcb, rxg.REC16, ntcb=ntcb)
    try:
        assert b.m == 7
        assert b.run(what="two scan rounds") == b.run(one_block, what="two scan rounds, max_blocks 1")
        b.run(cap=3, what="two scan rounds, cap 3")
        b.run(what="again after the cut call")
    finally:
        b.close()


def test_rec8_maximum_index(engine):
    b = crafted(engine, np.array([cases.REC8_MAX_TCB, 0, cases.REC8_MAX_TCB, -1]), rxg.REC8, ntcb=rxg.FS_MAX_NTCB)
    assert b.wcount.tolist() == [2, 1, 0]
    run_close(b, what="REC8's largest index")


# -------------------------------------- 4. record kinds, frame forms, the checksum flag ---
@pytest.fixture(scope="module")
def mixed_traffic():
    rng = np.random.default_rng(21)
    flow_of = np.where(rng.random(700) < 0.15, -1, rng.integers(0, 90, 700))
    return cases.table(90), cases.traffic(flow_of.tolist(), seed=8, bad_ck=0.1)


@pytest.mark.parametrize("flags", [0, rxg.FS_TCP_OK_ONLY])
@pytest.mark.parametrize("rec_kind", KINDS)
def test_record_kinds_list_and_stride(engine, mixed_traffic, rec_kind, flags):
    rows, frames = mixed_traffic
    b = Batch(engine, rec_kind, len(rows), frames=frames, rows=rows, flags=flags)
    try:
        assert (int(b.wcount[2]) > 10) == bool(flags) and b.m > 50
        a = b.run(what=f"list, records of {rec_kind}")
    finally:
        b.close()
    b = Batch(engine, rec_kind, len(rows), frames=frames, rows=rows, flags=flags, strided=True)
    try:
        assert a == b.run(what=f"stride, records of {rec_kind}", use_stride=True)
        assert a == b.run(what="the strided pool through its offset list")
    finally:
        b.close()


def test_rec48_without_frames_and_short_frames(engine):
    run_close(crafted(engine, np.random.default_rng(2).integers(0, 50, 500), rxg.REC48, no_frames=True),
              what="REC48, frames NULL")
    lens = [0] + list(range(38, 47)) + [54]
    r = cases.craft(np.arange(len(lens)) % 3, seq=0xA1B2C3D4, ack=0xE5F60718)
    for kind in (rxg.REC8, rxg.REC16):
        b = Batch(engine, kind, 3, rec48=r, frames=cases.frames_for(r, lens, fill=0xFF))
        assert int(b.want["max_seq"].max()) == 0xA1B2C3D4
        run_close(b, what="frames cut inside seq and ack")


def test_data_bytes_pass_2_to_the_32(engine):
    n = 70000
    r = cases.craft(np.full(n, 5), seq=np.arange(n), ack=1, datalen=rxg.TX_MAX_DATA)
    b = Batch(engine, rxg.REC48, 6, rec48=r, no_frames=True)
    assert int(b.want[0]["data_bytes"]) == n * 65481
    run_close(b, what="70 000 full segments of one flow")


# ------------------------------------------------------------ 5. the zero invariant ---
def test_back_to_back_calls_leave_nothing_behind(engine):
    import torch
    s = torch.cuda.Stream()
    rng = np.random.default_rng(6)
    small = crafted(engine, rng.integers(0, 40, 300), rxg.REC16, ntcb=40, seed=2)
    big = crafted(engine, rng.integers(0, 3 * TILE, 2000), rxg.REC8, ntcb=3 * TILE, seed=3)
    bigger = crafted(engine, rng.integers(0, 5 * TILE, 1000), rxg.REC48, ntcb=5 * TILE + 3, seed=4)
    try:
        big.run(cap=7, what="cap cuts the output")               # entries past cap must be cleared too
        small.run(what="after a cut call")
        big.run(what="the larger table again")
        bigger.run(cap=0, what="growth, nothing written")
        small.run(what="after growth")
        bigger.run(what="the largest again")
        # no host wait between calls, and a call on another stream in between
        outs = [small.outs(), big.outs(), bigger.outs(), small.outs()]
        small.call(engine, outs[0])
        big.call(engine, outs[1], stream=s.cuda_stream)
        bigger.call(engine, outs[2])
        small.call(engine, outs[3], stream=s.cuda_stream)
        engine.sync()
        engine.stream_sync(s.cuda_stream)
        for b, o, what in ((small, outs[0], "first"), (big, outs[1], "caller stream"), (bigger, outs[2], "third"),
                           (small, outs[3], "caller stream again")):
            b.check(o, what)
        for o in outs:
            o[0].free()
            o[1].free()
    finally:
        for b in (small, big, bigger):
            b.close()


# ----------------------------------------------------- 6. n == 0 and argument errors ---
def test_argument_errors_and_empty_bursts_write_nothing(engine):
    lib = rxg.load_library()
    b = crafted(engine, np.arange(100) % 7, rxg.REC16, ntcb=7)
    o = b.outs()
    out, count, cap = o
    try:
        def args(**kw):
            a = dict(frames=b.da.ptr, off64=b.do.ptr, len=b.dl.ptr, slot0=0, stride64=0, n=b.n, rec_kind=b.rec_kind,
                     recs=b.dr.ptr, ntcb=7, flags=0, out=out.ptr, cap=cap, count=count.ptr + 8)
            a.update(kw)
            return rxg.DevFlowSums(**a)
        bad = [(dict(recs=None), b"NULL"), (dict(count=None), b"NULL"), (dict(out=None), b"NULL"),
               (dict(frames=None), b"NULL"), (dict(len=None), b"NULL"),
               (dict(rec_kind=0), b"rec_kind"), (dict(rec_kind=32), b"rec_kind"),
               (dict(ntcb=0), b"ntcb"), (dict(ntcb=rxg.FS_MAX_NTCB + 1), b"ntcb"),
               (dict(flags=2), b"flags"), (dict(flags=0x80000001), b"flags"),
               (dict(frames=b.da.ptr + 8), b"alignment"), (dict(out=out.ptr + 4), b"alignment"),
               (dict(count=count.ptr + 12), b"alignment"), (dict(off64=b.do.ptr + 2), b"alignment"),
               (dict(len=b.dl.ptr + 1), b"alignment"), (dict(recs=b.dr.ptr + 8), b"alignment"),
               (dict(recs=b.dr.ptr + 4, rec_kind=rxg.REC8), b"alignment"),
               (dict(off64=None, stride64=0), b"stride64"),
               (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
               (dict(off64=None, slot0=0, stride64=0xFFFFFFFF, n=3), b"2^32")]
        for kw, why in bad:
            assert lib.rxg_flow_sums_dev(engine.ctx, C.byref(args(**kw)), None) == -EINVAL, kw
            assert why in lib.rxg_last_error(), (kw, lib.rxg_last_error())
        assert lib.rxg_flow_sums_dev(engine.ctx, None, None) == -EINVAL
        assert lib.rxg_flow_sums_dev(None, C.byref(args()), None) == -EINVAL
        engine.sync()
        assert (out.download(np.uint8, (cap + GUARD) * 40) == FILL).all()
        assert (count.download(np.uint8, 40) == FILL).all()
        # n == 0: count = {0, 0, 0} and nothing else, in either addressing mode; out NULL with cap 0 is fine
        for kw in (dict(n=0), dict(n=0, off64=None, stride64=4), dict(n=0, out=None, cap=0)):
            assert lib.rxg_flow_sums_dev(engine.ctx, C.byref(args(**kw)), None) == 0, lib.rxg_last_error()
            engine.sync()
            cw = count.download(np.uint64, 5)
            assert cw.tolist() == [0xA5A5A5A5A5A5A5A5, 0, 0, 0, 0xA5A5A5A5A5A5A5A5]
            assert (out.download(np.uint8, (cap + GUARD) * 40) == FILL).all()
            count.upload(np.full(40, FILL, np.uint8))
        # and the valid call works
        assert lib.rxg_flow_sums_dev(engine.ctx, C.byref(args()), None) == 0
        engine.sync()
        b.check(o)
    finally:
        out.free()
        count.free()
        b.close()


# ------------------------------------------------------------ 7. host and device agree ---
@pytest.mark.parametrize("which", ["parity", "imix"])
def test_host_and_device_agree(engine, which):
    if which == "parity":
        rows, frames = pktgen.parity_set(seed=31, n=3000)
        frames = [f for f in frames if len(f) <= 2048]
    else:
        rows, frames = cases.table(1000), cases.imix()
    for kind in KINDS:
        b = Batch(engine, kind, len(rows), frames=frames, rows=rows)
        try:
            assert b.m > (20 if which == "parity" else 900)
            dev = b.run(what=f"{which}, records of {kind}")
            recs = b.dr.download(np.uint8, b.n * kind)          # what the burst wrote
            sums, count = rxg.flow_sums_host(recs, kind, len(rows), frames)
            assert sums.tobytes() + count[:3].tobytes() == dev
        finally:
            b.close()


# --------------------------------------------------------------------- 8. the replay ---
def run_replay(eng, rows, frames, recs, on_segment=None, tcpswitch=None):
    lib = rxg.load_library()
    bufs = [C.create_string_buffer(f, max(len(f), 64)) for f in frames]
    addr = {C.addressof(x): i for i, x in enumerate(bufs)}
    model = Model(rows, eng)

    def switch(u, idx, st, tcp, ip, m):
        if tcpswitch:
            tcpswitch(addr[m], idx)
        model.handle(idx, st, frames[addr[m]])
        return 0

    ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(), rxg.HANDOFF_ADD_MAC(),
                         rxg.HANDOFF_SEND_RESET(), rxg.HANDOFF_ON_SEGMENT(on_segment) if on_segment else rxg.HANDOFF_ON_SEGMENT(),
                         rxg.HANDOFF_TCPSWITCH(switch))
    ptrs = (C.c_void_p * len(bufs))(*[C.addressof(x) for x in bufs])
    rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, len(bufs), 16)
    assert rc == 0, lib.rxg_last_error()
    return model


def test_replay_answers_for_counted_packets_only(replay_engine):
    eng = replay_engine
    lib = rxg.load_library()
    rows, frames = scenario(5, n=900)
    n = len(frames)
    exp, _, erows = sequential_reference(rows, frames)
    b = Batch(eng, rxg.REC16, len(rows), frames=frames, rows=rows)
    o = b.outs(cap=b.m - 2)                                  # the two highest flows are past cap
    try:
        b.call(eng, o)
        eng.sync()
        b.check(o)
        host = o[0].download(np.uint8, (b.m - 2) * 40).view(rxg.FLOW_SUM_DTYPE).copy()
        recs = b.dr.download(rxg.REC16_DTYPE, n)
        burst = b.rec48["c"]
        listed = set(host["tcb_idx"].tolist())
        changed = {i for i, (v, idx, st) in enumerate(exp)
                   if (v, idx, st) != (int(burst["verdict"][i]), int(burst["tcb_idx"][i]), int(burst["state"][i]))}
        assert len(changed) > 10
        assert eng.flow_sum_current() is None                # before the replay: nothing
        eng.flow_sums_attach(host.ctypes.data, len(host))
        assert eng.flow_sum_current() is None                # attached, but no replay runs
        seen = {}
        model = run_replay(eng, rows, frames, recs, tcpswitch=lambda i, idx: seen.__setitem__(i, eng.flow_sum_current()))
        assert model.rows == erows
        ones = 0
        for i, (v, idx, st) in enumerate(exp):
            if v != rxg.V_DISPATCH:
                assert i not in seen                         # no handler ran: nothing to ask
                continue
            was = burst[i]
            counted = int(was["verdict"]) == rxg.V_DISPATCH and int(was["tcb_idx"]) in listed
            if i in changed or not counted:
                assert seen[i] is None, i
            elif seen[i] is not None:
                s, pkt = seen[i]
                assert pkt == i and s == host[np.searchsorted(host["tcb_idx"], idx)] and int(s["tcb_idx"]) == idx, i
                ones += 1
            else:
                # an unchanged answer may still have been re-classified (its tuple was written): then 0
                assert int(rxg_stats(eng)[0]) > 0, i
        assert ones > 100
        past = [int(t) for t in b.want["tcb_idx"][-2:]]
        assert all(seen[i] is None for i in seen if int(burst["tcb_idx"][i]) in past)
        assert eng.flow_sum_current() is None                # the attachment ended with the replay
        p, k = C.c_void_p(), C.c_uint32()
        assert lib.rxg_flow_sum_current(eng.ctx, None, C.byref(k)) == -EINVAL
        assert lib.rxg_flow_sum_current(eng.ctx, C.byref(p), None) == -EINVAL
        assert lib.rxg_flow_sum_current(None, C.byref(p), C.byref(k)) == -EINVAL
        # a second replay without a new attach sees nothing
        eng.tcb_load(*pktgen.table_arrays(rows))
        eng.rx_burst_dev(b.da.ptr, b.do.ptr, b.dl.ptr, n, b.dr.ptr, rxg.REC16)
        eng.sync()
        seen.clear()
        run_replay(eng, rows, frames, recs, tcpswitch=lambda i, idx: seen.__setitem__(i, eng.flow_sum_current()))
        assert seen and all(v is None for v in seen.values())
        # attach refuses a list that does not ascend
        assert lib.rxg_flow_sums_attach(eng.ctx, host[::-1].copy().ctypes.data, len(host)) == -EINVAL
        assert lib.rxg_flow_sums_attach(eng.ctx, None, 1) == -EINVAL
        assert lib.rxg_flow_sums_attach(None, host.ctypes.data, 1) == -EINVAL
        assert lib.rxg_flow_sums_attach(eng.ctx, None, 0) == 0
    finally:
        o[0].free()
        o[1].free()
        b.close()


def rxg_stats(eng):
    out = (C.c_uint64 * 4)()
    assert rxg.load_library().rxg_replay_stats(eng.ctx, out) == 0
    return list(out)


def test_recipe_once_per_flow_equals_the_per_packet_loop(engine):
    """Without table writes: max_seq_received and the highest ack applied per TCB are the same
    whether on_segment works per packet or once per flow at first_idx."""
    rng = np.random.default_rng(17)
    rows = cases.table(60, listener=False)            # no listener, no FIN: no handler writes the table
    frames = cases.traffic(rng.integers(0, 60, 800).tolist(), seed=12, unknown=0.1, fin=0.0)
    b = Batch(engine, rxg.REC16, len(rows), frames=frames, rows=rows)
    o = b.outs()
    try:
        b.call(engine, o)
        engine.sync()
        b.check(o)
        host = o[0].download(np.uint8, b.m * 40).view(rxg.FLOW_SUM_DTYPE).copy()
        recs = b.dr.download(rxg.REC16_DTYPE, b.n)
        per_packet = {}                                   # the reference's loop: tcp_in.c:66-71 per frame
        for i, r in enumerate(b.rec48):
            if int(r["c"]["verdict"]) == rxg.V_DISPATCH:
                t = per_packet.setdefault(int(r["c"]["tcb_idx"]), [0, 0, 0])
                t[0], t[1], t[2] = max(t[0], int(r["seq"])), max(t[1], int(r["ack"])), t[2] + 1
        state, calls = {}, []

        def on_segment(u, idx, seq, ack):
            cur = engine.flow_sum_current()
            t = state.setdefault(idx, [0, 0, 0])
            if cur is None:                               # per-packet work, as today
                t[0], t[1], t[2] = max(t[0], seq), max(t[1], ack), t[2] + 1
                calls.append(idx)
            elif cur[1] == int(cur[0]["first_idx"]):      # once per flow
                t[0], t[1], t[2] = max(t[0], int(cur[0]["max_seq"])), max(t[1], int(cur[0]["max_ack"])), t[2] + int(cur[0]["frames"])
                calls.append(idx)

        engine.flow_sums_attach(host.ctypes.data, len(host))
        run_replay(engine, rows, frames, recs, on_segment=on_segment)
        assert state == per_packet and len(per_packet) > 50
        assert sorted(calls) == sorted(per_packet)        # one unit of work per flow
    finally:
        o[0].free()
        o[1].free()
        b.close()
