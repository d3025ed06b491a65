"""GPU: rxg_tx_reset_dev (the reset replies of a burst built on the device from its records)
and their use during the replay (rxg_reset_attach / rxg_reset_take) against the reference
model tests/txreset_ref.py -- a restatement of send_reset / ip_out / ether_out with the
oracle's checksums, itself pinned in tests/test_txreset_host.py -- never against the kernel's
own output.  The records are the ones a real rxg_rx_burst_dev of the same batch wrote; the
model is fed the verdicts of the CPU oracle.  Output pools, idx and count are pre-filled with
0xA5 and compared whole, guard slots past `cap` included."""
import ctypes as C
import random

import numpy as np
import pytest

import oracle
import pktgen
import rxg
import txreset_ref as ref
from test_gpu_replay import Model, sequential_reference

pytestmark = pytest.mark.gpu

FILL = 0xA5
FILL64 = 0xA5A5A5A5A5A5A5A5
GUARD = 8          # slots / entries past cap that must keep their fill
EINVAL = 22
SLICE = 64         # frames per slice of the kernel's count and build passes (rxg_txreset.hip)
DST = pktgen.ip4(192, 168, 78, 2)
MAC = bytes([0x02, 0xAB, 0xCD, 0xEF, 0x01, 0x99])


class Batch:
    """A batch on the device with the records of a real burst (kept alive until closed)."""

    def __init__(self, eng, arena, off, lens, rec_kind, tcb, live, off_dev=True):
        self.eng, self.n, self.rec_kind = eng, len(lens), rec_kind
        self.arena, self.off, self.lens = arena, np.asarray(off, np.uint32), np.asarray(lens, np.uint16)
        eng.tcb_load(tcb, live)
        n = max(self.n, 1)
        self.da, self.dl = eng.to_device(arena), eng.to_device(self.lens if self.n else np.zeros(1, np.uint16))
        self.do = eng.to_device(self.off if self.n else np.zeros(1, np.uint32))
        self.dr = eng.to_device(np.full(n * rec_kind, FILL, np.uint8))
        if self.n:
            eng.rx_burst_dev(self.da.ptr, self.do.ptr, self.dl.ptr, self.n, self.dr.ptr, rec_kind)
            eng.sync()
        self.verdicts = oracle.rx_batch(arena, self.off, self.lens, tcb, live)[0]["c"]["verdict"] if self.n \
            else np.zeros(0, np.uint8)

    def close(self):
        for d in (self.da, self.dl, self.do, self.dr):
            d.free()


class Out:
    """Output buffers of one call, pre-filled: cap + GUARD slots / entries, the count word."""

    def __init__(self, eng, cap):
        self.cap = cap
        self.out = eng.to_device(np.full((cap + GUARD) * 64, FILL, np.uint8))
        self.idx = eng.to_device(np.full((cap + GUARD) * 4, FILL, np.uint8))
        self.count = eng.to_device(np.full(8, FILL, np.uint8))

    def get(self):
        return (self.out.download(np.uint8, (self.cap + GUARD) * 64), self.idx.download(np.uint32, self.cap + GUARD),
                int(self.count.download(np.uint64, 1)[0]))

    def free(self):
        for d in (self.out, self.idx, self.count):
            d.free()


def call(eng, b, o, ip_id0=0, src_mac=MAC, stream=None, strided=None, lens_dev=None, arena_dev=None):
    eng.tx_reset_dev((arena_dev or b.da).ptr, (lens_dev or b.dl).ptr, b.n, b.dr.ptr, b.rec_kind, o.out.ptr, o.idx.ptr,
                     o.cap, o.count.ptr, off64=None if strided else b.do.ptr, slot0=strided[0] if strided else 0,
                     stride64=strided[1] if strided else 0, ip_id0=ip_id0, src_mac=src_mac, stream=stream)


def check(got, want, cap, what=""):
    """got: Out.get(); want: ref.build(..) for the same cap.  Everything compared: the built
    slots and entries, the fill past min(count, cap), the full count."""
    g_out, g_idx, g_count = got
    w_out, w_idx, w_count = want
    nb = min(w_count, cap)
    assert g_count == w_count, (what, g_count, w_count)
    assert len(w_idx) == nb
    assert np.array_equal(g_idx[:nb], w_idx), (what, "idx")
    assert (g_idx[nb:] == 0xA5A5A5A5).all(), (what, "idx entries at or past min(count, cap) were written")
    if not np.array_equal(g_out[:nb * 64], w_out):
        bad = np.nonzero(g_out[:nb * 64] != w_out)[0]
        k, byte = int(bad[0]) // 64, int(bad[0]) % 64
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first in reset {k} (packet {int(w_idx[k])}) byte {byte}: "
                             f"got {int(g_out[bad[0]]):#x} want {int(w_out[bad[0]]):#x}")
    assert (g_out[nb * 64:] == FILL).all(), (what, "slots at or past min(count, cap) were written")


def run(eng, b, cap, ip_id0=0, **kw):
    o = Out(eng, cap)
    try:
        call(eng, b, o, ip_id0, **kw)
        eng.sync()
        return o.get()
    finally:
        o.free()


# ------------------------------------------------------------------ 1. the parity set ---
@pytest.fixture(scope="module")
def parity():
    rows, frames = pktgen.parity_set(seed=41, n=3000)
    tcb, live = pktgen.table_arrays(rows)
    arena, off, lens = pktgen.pack_arena(frames)
    recs = oracle.rx_batch(arena, off, lens, tcb, live)[0]["c"]
    rst = np.isin(recs["verdict"], ref.RST_VERDICTS)
    # every edge kind is there, among the offenders too
    assert set(range(6)) <= set(recs["verdict"].tolist())
    assert (recs["flags"][rst] & rxg.F_TRUNC).any() and ((recs["flags"][rst] & rxg.F_TCP_OK) == 0).any()
    assert any(f[14] != 0x45 for f, r in zip(frames, rst) if r and len(f) >= 54)
    want = ref.build(arena, off, lens, recs["verdict"], 0x1234, MAC, len(frames))
    assert want[2] > 300
    # the same frames at a fixed stride, from slot 3
    stride64 = int((lens.max() + 63) // 64)
    slot0 = 3
    soff = (slot0 + np.arange(len(frames)) * stride64).astype(np.uint32)
    sarena = np.full((slot0 + len(frames) * stride64) * 64, 0x5A, np.uint8)
    for f, o in zip(frames, soff):
        sarena[int(o) * 64:int(o) * 64 + len(f)] = np.frombuffer(f, np.uint8)
    return dict(tcb=tcb, live=live, packed=(arena, off, lens), strided=(sarena, soff, lens), geom=(slot0, stride64),
                want=want, n=len(frames))


@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16, rxg.REC48])
def test_parity_set_every_record_kind_list_and_stride(engine, parity, rec_kind):
    n, want = parity["n"], parity["want"]
    b = Batch(engine, *parity["packed"], rec_kind, parity["tcb"], parity["live"])
    try:
        check(run(engine, b, n, 0x1234), want, n, "list")
    finally:
        b.close()
    b = Batch(engine, *parity["strided"], rec_kind, parity["tcb"], parity["live"])
    try:
        check(run(engine, b, n, 0x1234, strided=parity["geom"]), want, n, "strided")
        check(run(engine, b, n, 0x1234), want, n, "strided pool through its offset list")
    finally:
        b.close()


# -------------------------------------------------------------- 2. rank boundaries ---
NMAX = 4999
SIZES = [0, 1, 63, 64, 65, 3 * SLICE + 17, 1023, 1024, 1025, NMAX]


@pytest.fixture(scope="module")
def pool():
    """NMAX frames that get a reset (to a closed port; odd ones truncated or with IP options)
    and NMAX that do not (an established flow, an ARP request, UDP), of one to three slots."""
    rng = random.Random(5)
    rows = [(80, 0, pktgen.raw_of_host(DST), 0, pktgen.LISTENING)]
    flows = [(pktgen.ip4(10, 2, f >> 8, f & 255), 5000 + f) for f in range(50)]
    rows += [(80, sp, pktgen.raw_of_host(DST), src, pktgen.ESTABLISHED) for src, sp in flows]
    yes, no = [], []
    for k in range(NMAX):
        f = pktgen.frame(src_ip=pktgen.ip4(172, 16, k >> 8, k & 255), dst_ip=DST, sport=1024 + k, dport=9000 + k % 7,
                         seq=rng.getrandbits(32), ack=rng.getrandbits(32), flags=rng.choice([0x02, 0x10, 0x18, 0x11]),
                         payload=rng.randbytes(rng.choice([0, 6, 10, 11, 70, 90])), ihl=rng.choice([5, 5, 5, 6]),
                         src_mac=rng.randbytes(6))
        if k % 9 == 4:
            f = f[:rng.randrange(38, 54)]
        yes.append(f)
        src, sp = rng.choice(flows)
        no.append(rng.choice([
            pktgen.frame(src_ip=src, dst_ip=DST, sport=sp, dport=80, payload=rng.randbytes(rng.randrange(0, 120))),
            b"\xff" * 6 + rng.randbytes(6) + b"\x08\x06" + rng.randbytes(28),
            pktgen.frame(proto=17, payload=rng.randbytes(20))]))
    tcb, live = pktgen.table_arrays(rows)
    return dict(yes=yes, no=no, tcb=tcb, live=live)


def pattern(name, n):
    m = np.zeros(n, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "first" and n:
        m[0] = True
    elif name == "last" and n:
        m[-1] = True
    elif name == "sparse":
        m = np.random.default_rng(1000 + n).random(n) < 0.01
    return m


PATTERNS = ["all", "none", "alternating", "first", "last", "sparse"]


@pytest.fixture(scope="module")
def grids(engine):
    """Contexts whose launches are capped at 1 and 2 workgroups, and the occupancy grid."""
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    e1.close()
    e2.close()


@pytest.mark.parametrize("n", SIZES)
def test_rank_boundaries_and_grids(engine, pool, grids, n):
    for name in PATTERNS:
        m = pattern(name, n)
        frames = [pool["yes"][i] if m[i] else pool["no"][i] for i in range(n)]
        arena, off, lens = pktgen.pack_arena(frames)
        b = Batch(engine, arena, off, lens, rxg.REC8, pool["tcb"], pool["live"])
        try:
            assert np.array_equal(np.isin(b.verdicts, ref.RST_VERDICTS), m), name
            want = ref.build(arena, off, lens, b.verdicts, 7, MAC, n)
            assert want[2] == int(m.sum())
            for gname, eng in grids:
                check(run(eng, b, n, 7), want, n, f"{name}, n {n}, {gname}")
        finally:
            b.close()


# ------------------------------------------------------------- 3. truncated offenders ---
def test_truncated_offenders_read_as_zero(engine, pool):
    """A reset is built from the offender's bytes below len[i] only.  The records are a real
    burst's of the whole frames (a frame of 14 bytes has no protocol byte for the receive
    path to call it TCP); the reset call is then given shorter lengths -- it is a pure function
    of its arguments -- with the slot bytes from there to the line's end set to 0xFF."""
    cuts = [14, 34, 40, 46, 53]
    n = 400
    m = np.ones(n, dtype=bool)
    m[3::5] = False
    frames = [(pool["yes"][i] + bytes(64))[:64] if m[i] else pool["no"][i] for i in range(n)]
    # (the padding past a whole frame's end belongs to its IP payload: the verdict is the same)
    arena, off, lens = pktgen.pack_arena(frames)
    b = Batch(engine, arena, off, lens, rxg.REC16, pool["tcb"], pool["live"])
    try:
        assert np.array_equal(np.isin(b.verdicts, ref.RST_VERDICTS), m)
        short = lens.copy()
        poisoned = arena.copy()
        for k, i in enumerate(np.nonzero(m)[0]):
            short[i] = cuts[k % len(cuts)]
            a = int(off[i]) * 64
            poisoned[a + int(short[i]):a + 64] = 0xFF
        assert set(short[m].tolist()) == set(cuts)
        want = ref.build(arena, off, short, b.verdicts, 0, MAC, n)   # the model reads zeros past len
        assert want[0].tobytes() != ref.build(arena, off, lens, b.verdicts, 0, MAC, n)[0].tobytes()
        dp, ds = engine.to_device(poisoned), engine.to_device(short)
        try:
            check(run(engine, b, n, 0, arena_dev=dp, lens_dev=ds), want, n)
        finally:
            dp.free()
            ds.free()
    finally:
        b.close()


# ------------------------------------------------------------ 4. cap, 5. ip_id0 wrap ---
@pytest.fixture(scope="module")
def mixed(engine, pool):
    n = 700
    m = np.random.default_rng(3).random(n) < 0.4
    frames = [pool["yes"][i] if m[i] else pool["no"][i] for i in range(n)]
    arena, off, lens = pktgen.pack_arena(frames)
    b = Batch(engine, arena, off, lens, rxg.REC8, pool["tcb"], pool["live"])
    yield b
    b.close()


def test_cap_limits_what_is_written_not_the_count(engine, mixed):
    b = mixed
    count = int(np.isin(b.verdicts, ref.RST_VERDICTS).sum())
    assert count > 200
    for cap in (0, 1, count - 1, count, count + 7):
        want = ref.build(b.arena, b.off, b.lens, b.verdicts, 9, MAC, cap)
        assert want[2] == count and len(want[1]) == min(count, cap)
        check(run(engine, b, cap, 9), want, cap, f"cap {cap}")


@pytest.mark.parametrize("ip_id0", [0, 0xFFFE])
def test_ip_id_counts_up_and_wraps(engine, mixed, ip_id0):
    b = mixed
    want = ref.build(b.arena, b.off, b.lens, b.verdicts, ip_id0, MAC, b.n)
    got = run(engine, b, b.n, ip_id0)
    check(got, want, b.n)
    lines = got[0][:want[2] * 64].reshape(-1, 64)
    ids = lines[:, 18].astype(np.uint32) | (lines[:, 19].astype(np.uint32) << 8)
    assert ids[:3].tolist() == [ip_id0, (ip_id0 + 1) & 0xFFFF, (ip_id0 + 2) & 0xFFFF]
    assert np.array_equal(ids, (ip_id0 + np.arange(want[2])) & 0xFFFF)


# ------------------------------------------------- 6. two streams, one slice buffer ---
def test_two_streams_share_the_slice_counts(engine, pool):
    """Calls back to back on two streams of one (fresh) context, no host wait between them:
    the second call of each pair needs a larger slice-count buffer than the context has."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    small = [pool["yes"][i] if i % 2 else pool["no"][i] for i in range(1025)]
    big = [pool["yes"][i] if i % 3 else pool["no"][i] for i in range(NMAX)]
    bs = [Batch(engine, *pktgen.pack_arena(f), rxg.REC8, pool["tcb"], pool["live"]) for f in (small, big)]
    with rxg.Engine(device=0) as eng:
        order = [(0, s1), (1, s2), (0, s2), (1, s1), (0, s1)]
        outs = [Out(eng, bs[j].n) for j, _ in order]
        try:
            for (j, s), o in zip(order, outs):
                call(eng, bs[j], o, 5 + j, stream=s.cuda_stream)
            eng.stream_sync(s1.cuda_stream)
            eng.stream_sync(s2.cuda_stream)
            wants = [ref.build(b.arena, b.off, b.lens, b.verdicts, 5 + j, MAC, b.n) for j, b in enumerate(bs)]
            for (j, _), o in zip(order, outs):
                check(o.get(), wants[j], bs[j].n, f"batch {j}")
        finally:
            for o in outs:
                o.free()
            for b in bs:
                b.close()


# --------------------------------------------------------------- 7. argument errors ---
def test_argument_errors_launch_nothing(engine, mixed):
    lib = rxg.load_library()
    b = mixed
    o = Out(engine, b.n)
    try:
        def args(**kw):
            a = dict(frames=b.da.ptr, off64=b.do.ptr, len=b.dl.ptr, slot0=0, stride64=0, n=b.n, rec_kind=b.rec_kind,
                     recs=b.dr.ptr, out=o.out.ptr, idx=o.idx.ptr, cap=b.n, count=o.count.ptr, ip_id0=0,
                     src_mac=(C.c_uint8 * 6)(*MAC))
            a.update(kw)
            return rxg.DevTxReset(**a)
        bad = [(dict(frames=None), b"NULL"), (dict(len=None), b"NULL"), (dict(recs=None), b"NULL"),
               (dict(out=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(count=None), b"NULL"),
               (dict(rec_kind=0), b"rec_kind"), (dict(rec_kind=32), b"rec_kind"),
               (dict(frames=b.da.ptr + 8), b"alignment"), (dict(out=o.out.ptr + 32), b"alignment"),
               (dict(out=o.out.ptr + 16), b"alignment"), (dict(idx=o.idx.ptr + 2), b"alignment"),
               (dict(off64=b.do.ptr + 2), b"alignment"), (dict(len=b.dl.ptr + 1), b"alignment"),
               (dict(count=o.count.ptr + 4), b"alignment"), (dict(recs=b.dr.ptr + 4), b"alignment"),
               (dict(recs=b.dr.ptr + 8, rec_kind=rxg.REC16), b"alignment"),
               (dict(recs=b.dr.ptr + 8, rec_kind=rxg.REC48), b"alignment"),
               (dict(off64=None, stride64=0), b"stride64"),
               (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
               (dict(off64=None, slot0=0, stride64=0xFFFFFFFF, n=3), b"2^32")]
        for kw, why in bad:
            assert lib.rxg_tx_reset_dev(engine.ctx, C.byref(args(**kw)), None) == -EINVAL, kw
            assert why in lib.rxg_last_error(), (kw, lib.rxg_last_error())
        assert lib.rxg_tx_reset_dev(engine.ctx, None, None) == -EINVAL
        assert lib.rxg_tx_reset_dev(None, C.byref(args()), None) == -EINVAL
        engine.sync()
        g_out, g_idx, g_count = o.get()
        assert (g_out == FILL).all() and (g_idx == 0xA5A5A5A5).all() and g_count == FILL64
        # n == 0 writes *count = 0 and nothing else, in either addressing mode
        fill8 = np.full(8, FILL, np.uint8)
        for kw in (dict(n=0), dict(n=0, off64=None, stride64=4)):
            engine.h2d(o.count.ptr, fill8.ctypes.data, 8)
            engine.sync()
            assert lib.rxg_tx_reset_dev(engine.ctx, C.byref(args(**kw)), None) == 0, lib.rxg_last_error()
            engine.sync()
            g_out, g_idx, g_count = o.get()
            assert (g_out == FILL).all() and (g_idx == 0xA5A5A5A5).all() and g_count == 0
        # and the valid call works
        assert lib.rxg_tx_reset_dev(engine.ctx, C.byref(args()), None) == 0
        engine.sync()
        check(o.get(), ref.build(b.arena, b.off, b.lens, b.verdicts, 0, MAC, b.n), b.n)
    finally:
        o.free()


# --------------------------------------------------------------------- 8. the replay ---
LISTENING, ESTABLISHED = 1, 4


def replay_scenario(seed=17, n=900):
    """A listener on :80, established flows on :7000 (no listener there), and
      - clients that send a SYN to :80 and then ACKs: the ACKs are LISTEN_NONSYN resets at
        burst time and DISPATCH once the SYN's handler has added the child TCB;
      - flows that send a FIN and go on talking: closed, removed, then RST_NOPCB -- resets the
        burst did not see;
      - strangers to :80 without a SYN and to a closed port: resets then and now."""
    rng = random.Random(seed)
    raw = pktgen.raw_of_host(DST)
    rows = [(80, 0, raw, 0, LISTENING)]
    flows = [(pktgen.ip4(10, 3, 0, f), 3000 + f) for f in range(12)]
    rows += [(7000, sp, raw, src, ESTABLISHED) for src, sp in flows]
    clients = [(pktgen.ip4(172, 20, 0, c), 41000 + c) for c in range(25)]
    syn_sent = set()
    frames = []
    for _ in range(n):
        k = rng.random()
        kw = dict(dst_ip=DST, seq=rng.getrandbits(32), ack=rng.getrandbits(32), payload=rng.randbytes(rng.randrange(0, 40)),
                  src_mac=rng.randbytes(6))
        if k < 0.30:
            frames.append(pktgen.frame(src_ip=pktgen.ip4(172, 30, rng.randrange(256), rng.randrange(256)),
                                       sport=rng.randrange(1024, 65536), dport=9999, flags=rng.choice([0x02, 0x10]), **kw))
        elif k < 0.45:
            frames.append(pktgen.frame(src_ip=pktgen.ip4(172, 31, 0, rng.randrange(256)), sport=rng.randrange(1024, 65536),
                                       dport=80, flags=0x10, **kw))
        elif k < 0.65:
            c = rng.choice(clients)
            fl = 0x10 if c in syn_sent else 0x02
            syn_sent.add(c)
            frames.append(pktgen.frame(src_ip=c[0], sport=c[1], dport=80, flags=fl, **kw))
        elif k < 0.92:
            src, sp = rng.choice(flows)
            frames.append(pktgen.frame(src_ip=src, sport=sp, dport=7000, flags=0x11 if rng.random() < 0.12 else 0x10, **kw))
        else:
            frames.append(b"\xff" * 6 + rng.randbytes(6) + b"\x08\x06" + rng.randbytes(28))
    return rows, frames


def test_replay_hands_out_the_prebuilt_resets(replay_engine):
    eng = replay_engine
    lib = rxg.load_library()
    rows, frames = replay_scenario()
    n = len(frames)
    exp, _, erows = sequential_reference(rows, frames)
    tcb, live = pktgen.table_arrays(rows)
    arena, off, lens = pktgen.pack_arena(frames)
    ID0 = 0xFFF0
    b = Batch(eng, arena, off, lens, rxg.REC16, tcb, live)
    o = Out(eng, n)
    try:
        call(eng, b, o, ID0, src_mac=rxg.REF_SRC_MAC)
        eng.sync()
        g_out, g_idx, count = o.get()
        check((g_out, g_idx, count), ref.build(arena, off, lens, b.verdicts, ID0, rxg.REF_SRC_MAC, n), n)
        recs = b.dr.download(rxg.REC16_DTYPE, n)
        resets_host = np.ascontiguousarray(g_out[:count * 64])
        idx_host = np.ascontiguousarray(g_idx[:count])
        prebuilt = set(idx_host.tolist())
        seq_rst = [i for i, (v, _, _) in enumerate(exp) if v in ref.RST_VERDICTS]
        # the scenario bites: prebuilt resets no longer wanted, and resets the burst did not see
        dropped = sorted(i for i in prebuilt if exp[i][0] == rxg.V_DISPATCH)
        fresh = [i for i in seq_rst if i not in prebuilt]
        assert len(dropped) > 10 and len(fresh) > 10
        assert any(exp[i][0] == rxg.V_RST_NOPCB and b.verdicts[i] == rxg.V_DISPATCH for i in fresh)
        assert any(i > dropped[0] and i in prebuilt for i in seq_rst)

        eng.reset_attach(resets_host.ctypes.data, idx_host.ctypes.data, count)
        model = Model(rows, eng)
        bufs = [C.create_string_buffer(f, max(len(f), 64)) for f in frames]
        addr = {C.addressof(x): i for i, x in enumerate(bufs)}
        state = {"id": ID0}
        sent = []  # (packet, id passed, frame bytes, taken)

        def send_reset(u, ip, tcp):
            i = addr[ip - 14]
            ip_id = state["id"]
            p = eng.reset_take(ip_id)
            frame = C.string_at(p, 64) if p else ref.one(ref.offender_line(arena, off[i], lens[i]), ip_id)
            sent.append((i, ip_id, frame, p is not None))
            state["id"] = (ip_id + 1) & 0xFFFF   # ip_out's count++ (ip.c:106)

        def tcpswitch(u, idx, st, tcp, ip, m):
            model.handle(idx, st, frames[addr[m]])
            if st == LISTENING:                  # tcp_listen answers with a SYN-ACK: count++ again
                state["id"] = (state["id"] + 1) & 0xFFFF
            return 0

        ops = rxg.HandoffOps(None, rxg.HANDOFF_FREE(), rxg.HANDOFF_ARP_IN(), rxg.HANDOFF_GET_MAC(), rxg.HANDOFF_ADD_MAC(),
                             rxg.HANDOFF_SEND_RESET(send_reset), rxg.HANDOFF_ON_SEGMENT(), rxg.HANDOFF_TCPSWITCH(tcpswitch))
        ptrs = (C.c_void_p * n)(*[C.addressof(x) for x in bufs])
        rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n, 16)
        assert rc == 0, lib.rxg_last_error()
        assert model.rows == erows
        # the ids the reference's count++ gives, from the sequential oracle's verdicts alone
        want_ids, cur = {}, ID0
        for i, (v, idx, st) in enumerate(exp):
            if v in ref.RST_VERDICTS:
                want_ids[i] = cur
                cur = (cur + 1) & 0xFFFF
            elif v == rxg.V_DISPATCH and st == LISTENING:
                cur = (cur + 1) & 0xFFFF
        assert [s[0] for s in sent] == seq_rst
        assert [s[1] for s in sent] == [want_ids[i] for i in seq_rst]
        kpos = {int(p): k for k, p in enumerate(idx_host)}
        drift = 0
        for i, ip_id, frame, taken in sent:
            assert taken == (i in prebuilt), (i, taken)
            assert frame == ref.one(ref.offender_line(arena, off[i], lens[i]), ip_id), i
            if taken:
                drift += ip_id != (ID0 + kpos[i]) & 0xFFFF
        assert 0 < drift < sum(s[3] for s in sent)  # both: the id as built, and rxg_reset_set_id's
        assert any(s2[1] < s1[1] for s1, s2 in zip(sent, sent[1:]))  # the id wrapped at 16 bits
        # the attachment ended with the replay
        assert eng.reset_take(0) is None
        p = C.c_void_p()
        assert lib.rxg_reset_take(eng.ctx, 0, None) == -EINVAL
        rc = lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n - 1, 16)
        assert rc == -EINVAL  # a refused replay ends an attachment too
        eng.reset_attach(resets_host.ctypes.data, idx_host.ctypes.data, count)
        assert lib.rxg_rx_replay(eng.ctx, C.byref(ops), ptrs, ptrs, recs.ctypes.data, n - 1, 16) == -EINVAL
        assert lib.rxg_reset_take(eng.ctx, 0, C.byref(p)) == 0
    finally:
        o.free()
        b.close()
