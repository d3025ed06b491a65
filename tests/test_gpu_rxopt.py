"""GPU: rxg_rx_opts_dev (the TCP options of a burst's segments parsed on the device) and their
use during the replay (rxg_rx_opts_attach / rxg_rx_opt_current) against the model
tests/rxopt_ref.py -- a Python restatement of the rule in include/rxg.h, pinned in
tests/test_rxopt_host.py -- never against the kernel's own output or the host parser alone.
The records are the ones a real rxg_rx_burst_dev of the same batch wrote; the model is fed the
verdicts of the CPU oracle.  Output buffers are pre-filled with 0xA5 and compared whole, eight
guard records past n included; what follows a frame's last byte in the pool parses as valid
options (rxopt_cases.poisoned_arena), so a read at or beyond len shows in the record."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle
import pktgen
import rxg
import rxopt_cases as cases
import rxopt_ref as ref
from test_gpu_replay import Model, scenario, sequential_reference

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 8
EINVAL = 22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "rxopt_kat.json")))


def strided_pool(frames, slot0=3):
    """The frames at a fixed stride from slot0; everything that is not a frame byte holds the
    poison, in each frame's own phase."""
    lens = np.array([len(f) for f in frames], np.uint16)
    stride64 = max(1, (int(lens.max()) + 63) // 64)
    off = (slot0 + np.arange(len(frames)) * stride64).astype(np.uint32)
    arena = np.zeros((slot0 + len(frames) * stride64) * 64, np.uint8)
    x = np.arange(stride64 * 64)
    fill = np.frombuffer(cases.POISON, np.uint8)[(x - 54) % 16]
    arena[:slot0 * 64] = 0x08
    for f, o in zip(frames, off.tolist()):
        arena[o * 64:(o + stride64) * 64] = fill
        arena[o * 64:o * 64 + len(f)] = np.frombuffer(f, np.uint8)
    return arena, off, lens, (slot0, stride64)


class Batch:
    """A batch on the device with the records of a real burst (kept alive until closed)."""

    def __init__(self, eng, frames, rec_kind=rxg.REC8, table=None, strided=False):
        self.eng, self.frames, self.n, self.rec_kind = eng, frames, len(frames), rec_kind
        tcb, live = table if table is not None else cases.table()
        self.geom = None
        if strided:
            self.arena, self.off, self.lens, self.geom = strided_pool(frames)
        else:
            self.arena, self.off, self.lens = cases.poisoned_arena(frames)
        eng.tcb_load(tcb, live)
        n = max(self.n, 1)
        self.da = eng.to_device(self.arena)
        self.dl = eng.to_device(self.lens if self.n else np.zeros(1, np.uint16))
        self.do = eng.to_device(self.off if self.n else np.zeros(1, np.uint32))
        self.dr = eng.to_device(np.full(n * rec_kind, FILL, np.uint8))
        if self.n:
            eng.rx_burst_dev(self.da.ptr, self.do.ptr, self.dl.ptr, self.n, self.dr.ptr, rec_kind)
            eng.sync()
            self.verdicts = oracle.rx_batch(self.arena, self.off, self.lens, tcb, live)[0]["c"]["verdict"]
        else:
            self.verdicts = np.zeros(0, np.uint8)
        self.want = ref.records(frames, self.verdicts)

    def out(self):
        return self.eng.to_device(np.full((self.n + GUARD) * 16, FILL, np.uint8))

    def call(self, eng, out, use_stride=False, stream=None):
        eng.rx_opts_dev(self.da.ptr, self.dl.ptr, self.n, self.dr.ptr, self.rec_kind, out.ptr,
                        off64=None if use_stride else self.do.ptr, slot0=self.geom[0] if use_stride else 0,
                        stride64=self.geom[1] if use_stride else 0, stream=stream)

    def check(self, out, what=""):
        raw = out.download(np.uint8, (self.n + GUARD) * 16)
        assert (raw[self.n * 16:] == FILL).all(), (what, "records past n were written")
        got = raw[:self.n * 16].view(rxg.RX_OPT_DTYPE)
        if not np.array_equal(got, self.want):
            bad = np.nonzero(got != self.want)[0]
            i = int(bad[0])
            raise AssertionError(f"{what}: {len(bad)} of {self.n} records differ, first at packet {i} (len "
                                 f"{len(self.frames[i])}, verdict {int(self.verdicts[i])}, bytes 46.. "
                                 f"{self.frames[i][46:94].hex()}): got {got[i]} want {self.want[i]}")
        return raw

    def run(self, eng=None, what="", **kw):
        eng = eng or self.eng
        o = self.out()
        try:
            self.call(eng, o, **kw)
            eng.sync()
            return self.check(o, what)
        finally:
            o.free()

    def close(self):
        for d in (self.da, self.dl, self.do, self.dr):
            d.free()


# ------------------------------------------------------------ 1. the vectors and the sets ---
def test_known_answers(engine):
    frames = [cases.seg(bytes.fromhex(k["opts"]), payload=b"\x08\x0a" * 8) for k in KATS]
    b = Batch(engine, frames)
    try:
        assert (b.verdicts == rxg.V_DISPATCH).all()
        for k, w in zip(KATS, b.want):    # the model's records are the hand-written ones
            assert ref.as_tuple(w) == tuple(k["want"][f] for f in ref.FIELDS), k["name"]
        b.run(what="vectors")
    finally:
        b.close()


@pytest.fixture(scope="module")
def sets():
    return {name: fn() for name, fn in cases.SETS.items()}


@pytest.mark.parametrize("name", list(cases.SETS))
def test_sets_equal_the_model(engine, sets, name):
    frames = sets[name]
    table = pktgen.table_arrays(pktgen.parity_set(31, 1)[0]) if name == "parity" else None
    b = Batch(engine, frames, table=table)
    try:
        cand = np.isin(b.verdicts, ref.CANDIDATE_VERDICTS)
        if name == "zero_records":
            short = np.array([len(f) < 24 for f in frames])
            assert not cand[:5].any() and not cand[short].any() and short.sum() >= 4
            assert not b.want[~cand].view(np.uint8).any()
        elif name == "random_tlv":
            assert set(ref.CANDIDATE_VERDICTS) <= set(b.verdicts.tolist())
        elif name == "parity":
            assert set(range(6)) <= set(b.verdicts.tolist()) and (b.want["flags"] & rxg.O_CUT).any()
        else:
            assert cand.all()
        if name == "cut_frames":   # the pool ends with the line of the 60-byte frame claiming 40 option bytes
            assert len(frames[-1]) == 60 and frames[-1][46] >> 4 == 15 and len(b.arena) == (int(b.off[-1]) + 1) * 64
        b.run(what=name)
    finally:
        b.close()


# ----------------------------------------- 2. record kinds, offset list and fixed stride ---
@pytest.fixture(scope="module")
def blend(sets):
    return sets["cut_frames"] + sets["random_tlv"][:700] + sets["zero_records"] + sets["slices"][:200] + sets["parity"][:300]


@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16, rxg.REC48])
def test_record_kinds_list_and_stride(engine, blend, rec_kind):
    frames = [f for f in blend if len(f) <= 2048]
    b = Batch(engine, frames, rec_kind)
    try:
        b.run(what=f"list, records of {rec_kind}")
    finally:
        b.close()
    b = Batch(engine, frames, rec_kind, strided=True)
    try:
        b.run(what=f"stride, records of {rec_kind}", use_stride=True)
        b.run(what="the strided pool through its offset list")
    finally:
        b.close()


# --------------------------------------------------------------- 3. sizes and the grid ---
@pytest.fixture(scope="module")
def grids(engine):
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    e1.close()
    e2.close()


@pytest.mark.parametrize("n", cases.SIZES)
def test_sizes_on_every_grid(engine, grids, n):
    b = Batch(engine, cases.mixed(257)[:n])
    try:
        raws = [b.run(eng, f"n {n}, {gname}").tobytes() for gname, eng in grids]
        assert raws[0] == raws[1] == raws[2]
    finally:
        b.close()


def test_grids_give_identical_bytes(engine, grids, sets):
    b = Batch(engine, sets["slices"] + sets["random_tlv"][:1500] + sets["boundaries"])
    try:
        raws = [b.run(eng, gname).tobytes() for gname, eng in grids]
        assert raws[0] == raws[1] == raws[2]
    finally:
        b.close()


# ------------------------------------------- 4. a caller stream, two calls back to back ---
def test_caller_stream_and_back_to_back_calls(engine, sets):
    import torch
    s = torch.cuda.Stream()
    b1, b2 = Batch(engine, sets["random_tlv"][:1000]), Batch(engine, sets["slices"], rxg.REC16)
    outs = [b1.out(), b2.out(), b1.out(), b2.out()]
    try:
        b1.call(engine, outs[0])
        b2.call(engine, outs[1])                      # no host wait between the two
        b1.call(engine, outs[2], stream=s.cuda_stream)
        b2.call(engine, outs[3], stream=s.cuda_stream)
        engine.sync()
        engine.stream_sync(s.cuda_stream)
        for b, o, what in ((b1, outs[0], "first"), (b2, outs[1], "second"), (b1, outs[2], "first, caller stream"),
                           (b2, outs[3], "second, caller stream")):
            b.check(o, what)
    finally:
        for o in outs:
            o.free()
        b1.close()
        b2.close()


# --------------------------------------------------------------- 5. argument errors ---
def test_argument_errors_launch_nothing(engine, sets):
    lib = rxg.load_library()
    b = Batch(engine, sets["random_tlv"][:300])
    o = b.out()
    try:
        def args(**kw):
            a = dict(frames=b.da.ptr, off64=b.do.ptr, len=b.dl.ptr, slot0=0, stride64=0, n=b.n, rec_kind=b.rec_kind,
                     recs=b.dr.ptr, out=o.ptr)
            a.update(kw)
            return rxg.DevRxOpts(**a)
        bad = [(dict(frames=None), b"NULL"), (dict(len=None), b"NULL"), (dict(recs=None), b"NULL"), (dict(out=None), b"NULL"),
               (dict(rec_kind=0), b"rec_kind"), (dict(rec_kind=32), b"rec_kind"),
               (dict(frames=b.da.ptr + 8), b"alignment"), (dict(out=o.ptr + 8), b"alignment"),
               (dict(out=o.ptr + 4), b"alignment"), (dict(off64=b.do.ptr + 2), b"alignment"),
               (dict(len=b.dl.ptr + 1), b"alignment"), (dict(recs=b.dr.ptr + 4), b"alignment"),
               (dict(recs=b.dr.ptr + 8, rec_kind=rxg.REC16), b"alignment"),
               (dict(recs=b.dr.ptr + 8, rec_kind=rxg.REC48), b"alignment"),
               (dict(off64=None, stride64=0), b"stride64"),
               (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
               (dict(off64=None, slot0=0, stride64=0xFFFFFFFF, n=3), b"2^32")]
        for kw, why in bad:
            assert lib.rxg_rx_opts_dev(engine.ctx, C.byref(args(**kw)), None) == -EINVAL, kw
            assert why in lib.rxg_last_error(), (kw, lib.rxg_last_error())
        assert lib.rxg_rx_opts_dev(engine.ctx, None, None) == -EINVAL
        assert lib.rxg_rx_opts_dev(None, C.byref(args()), None) == -EINVAL
        # n == 0 launches nothing and writes nothing, in either addressing mode
        for kw in (dict(n=0), dict(n=0, off64=None, stride64=4)):
            assert lib.rxg_rx_opts_dev(engine.ctx, C.byref(args(**kw)), None) == 0, lib.rxg_last_error()
        engine.sync()
        assert (o.download(np.uint8, (b.n + GUARD) * 16) == FILL).all()
        # and the valid call works
        assert lib.rxg_rx_opts_dev(engine.ctx, C.byref(args()), None) == 0
        engine.sync()
        b.check(o)
    finally:
        o.free()
        b.close()


# ------------------------------------------------ 6. round trip with the transmit build ---
def test_round_trip_with_the_tx_option_build(engine):
    """Segments built by rxg_tx_build_opt_dev with the timestamp block, the reference ACK's
    block and a SYN block, mixed with option-less ones, classified and parsed on the device:
    what comes out is what went in."""
    n = 600
    syn = cases.mss(1460) + cases.sack_perm() + cases.timestamp(0xCAFE0001, 0) + cases.NOP + cases.wscale(7)
    blocks = [rxg.tx_opt_timestamp(0x10000000 + k, 0xFFFFFFF0 + k) for k in range(20)]
    blocks += [rxg.tx_opt_ref_ack(), rxg.tx_opt_set(syn)]
    opts = np.concatenate([np.atleast_1d(x) for x in blocks]).astype(rxg.TX_OPT_DTYPE)
    flows = np.zeros(1, rxg.TX_FLOW_DTYPE)
    flows[0]["dport"], flows[0]["sport"] = 80, 40000
    flows[0]["ipv4_dst"], flows[0]["ipv4_src"] = pktgen.raw_of_host(cases.DST), pktgen.ip4(10, 9, 8, 7)
    rng = np.random.default_rng(9)
    segs = np.zeros(n, rxg.TX_SEG_DTYPE)
    segs["reserved"] = rng.integers(0, len(opts) + 1, n)
    segs["reserved"][::7] = 0
    segs["data_len"] = rng.choice([0, 1, 10, 22, 100, 1448 - 12], n)
    segs["src_off"] = rng.integers(0, 2000, n)
    segs["seq"], segs["ack"] = rng.integers(0, 2**32, n), rng.integers(0, 2**32, n)
    segs["tcp_flags"] = np.where(segs["reserved"] == len(opts), 0x02, 0x10)
    stride64 = (54 + 40 + 1448 + 63) // 64
    arena, lens, stats = engine.tx_build(rng.integers(0, 256, 4096, dtype=np.uint8), flows, segs, slot0=0, stride64=stride64,
                                         opts=opts)
    assert int(stats[0]) == n and int(stats[1]) == 0
    used = sorted(set(segs["reserved"].tolist()))
    assert used[0] == 0 and {1, len(opts) - 1, len(opts)} <= set(used)
    tcb, live = pktgen.table_arrays([])
    engine.tcb_load(tcb, live)
    da, dl = engine.to_device(arena), engine.to_device(lens)
    dr, out = engine.to_device(np.full(n * 8, FILL, np.uint8)), engine.to_device(np.full((n + GUARD) * 16, FILL, np.uint8))
    try:
        engine.rx_bursts_strided_dev(da.ptr, stride64, [(0, dl.ptr, n, dr.ptr)], rxg.REC8)
        engine.rx_opts_dev(da.ptr, dl.ptr, n, dr.ptr, rxg.REC8, out.ptr, off64=None, slot0=0, stride64=stride64)
        engine.sync()
        raw = out.download(np.uint8, (n + GUARD) * 16)
        assert (raw[n * 16:] == FILL).all()
        got = raw[:n * 16].view(rxg.RX_OPT_DTYPE)
        frames = [arena[i * stride64 * 64:i * stride64 * 64 + int(lens[i])].tobytes() for i in range(n)]
        assert np.array_equal(got, ref.records(frames, np.full(n, rxg.V_RST_NOPCB)))   # the model, on the built frames
        for i in range(n):                                                            # and what went in
            k = int(segs["reserved"][i])
            g = got[i]
            if k == 0:
                assert ref.as_tuple(g) == (0, 0, 0, 0, 0, 0, 0, rxg.O_PARSED), i
                continue
            assert int(g["opt_len"]) == int(opts[k - 1]["len"]), i
            if k <= 20:
                want = (0x10000000 + k - 1, (0xFFFFFFF0 + k - 1) & 0xFFFFFFFF, 0, 0, rxg.O_PARSED | rxg.O_TS)
            elif k == 21:
                want = (0x18190300, 0, 1300, 7, rxg.O_PARSED | rxg.O_TS | rxg.O_MSS | rxg.O_WSCALE)
            else:
                want = (0xCAFE0001, 0, 1460, 7, rxg.O_PARSED | rxg.O_TS | rxg.O_MSS | rxg.O_WSCALE | rxg.O_SACK_PERM)
            assert (int(g["tsval"]), int(g["tsecr"]), int(g["mss"]), int(g["wscale"]), int(g["flags"])) == want, (i, k)
    finally:
        for d in (da, dl, dr, out):
            d.free()


# --------------------------------------------------------------------- 7. the replay ---
def test_replay_hands_out_each_packets_record(replay_engine):
    eng = replay_engine
    lib = rxg.load_library()
    rows, plain = scenario(5, n=900)
    # every frame gets the aligned timestamp with its own packet number as tsval (the 4-tuple,
    # the flags and so the verdicts stay what they were)
    frames = [f[:46] + b"\x80" + f[47:54] + cases.aligned_ts(i, 0xABCD0000 + i) + f[54:] for i, f in enumerate(plain)]
    n = len(frames)
    exp, _, erows = sequential_reference(rows, frames)
    b = Batch(eng, frames, rxg.REC16, table=pktgen.table_arrays(rows))
    o = b.out()
    try:
        b.call(eng, o)
        eng.sync()
        host = np.ascontiguousarray(b.check(o)[:n * 16]).view(rxg.RX_OPT_DTYPE)
        assert (host["tsval"] == np.arange(n)).all() and (host["flags"] == rxg.O_PARSED | rxg.O_TS).all()
        recs = b.dr.download(rxg.REC16_DTYPE, n)
        changed = [i for i, (v, _, _) in enumerate(exp) if v != int(b.verdicts[i])]
        assert len(changed) > 10   # packets the replay re-classifies
        assert eng.rx_opt_current() is None                        # before the replay: nothing
        eng.rx_opts_attach(host.ctypes.data, n)
        assert eng.rx_opt_current() is None                        # attached, but no replay runs
        model = Model(rows, eng)
        bufs = [C.create_string_buffer(f, max(len(f), 64)) for f in frames]
        addr = {C.addressof(x): i for i, x in enumerate(bufs)}
        seen = []

        def send_reset(u, ip, tcp):
            seen.append((addr[ip - 14], eng.rx_opt_current()))

        def tcpswitch(u, idx, st, tcp, ip, m):
            seen.append((addr[m], eng.rx_opt_current()))
            model.handle(idx, st, frames[addr[m]])
            return 0

        ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(), rxg.HANDOFF_ADD_MAC(),
                             rxg.HANDOFF_SEND_RESET(send_reset), rxg.HANDOFF_ON_SEGMENT(), rxg.HANDOFF_TCPSWITCH(tcpswitch))
        ptrs = (C.c_void_p * n)(*[C.addressof(x) for x in bufs])
        rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n, 16)
        assert rc == 0, lib.rxg_last_error()
        assert model.rows == erows
        assert [i for i, _ in seen] == list(range(n))                # every packet is TCP here
        for i, r in seen:
            assert r is not None and ref.as_tuple(r) == ref.as_tuple(b.want[i]) and int(r["tsval"]) == i, i
        assert set(changed) <= {i for i, _ in seen}
        # the attachment ended with the replay
        assert eng.rx_opt_current() is None
        p = C.c_void_p()
        assert lib.rxg_rx_opt_current(eng.ctx, None) == -EINVAL
        # a second replay without a new attach sees nothing
        eng.tcb_load(*pktgen.table_arrays(rows))
        eng.rx_burst_dev(b.da.ptr, b.do.ptr, b.dl.ptr, n, b.dr.ptr, rxg.REC16)
        eng.sync()
        recs = b.dr.download(rxg.REC16_DTYPE, n)
        seen.clear()
        model = Model(rows, eng)
        rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n, 16)
        assert rc == 0, lib.rxg_last_error()
        assert len(seen) == n and all(r is None for _, r in seen)
        # an attachment of another size answers nothing either, and ends with its replay
        eng.tcb_load(*pktgen.table_arrays(rows))
        eng.rx_burst_dev(b.da.ptr, b.do.ptr, b.dl.ptr, n, b.dr.ptr, rxg.REC16)
        eng.sync()
        eng.rx_opts_attach(host.ctypes.data, n - 1)
        seen.clear()
        model = Model(rows, eng)
        rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n, 16)
        assert rc == 0 and len(seen) == n and all(r is None for _, r in seen)
        assert lib.rxg_rx_opt_current(eng.ctx, C.byref(p)) == 0
    finally:
        o.free()
        b.close()
