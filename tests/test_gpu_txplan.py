"""GPU: rxg_tx_plan_dev (sends cut into segment descriptors on the device) against the shipped host
planner through tests/txplan_cases.expect -- never against the kernel's own output.  Every device
buffer is pre-filled with 0xA5 and compared whole: segs carries eight guard descriptors behind
`cap`, first and next_seq eight guard entries behind their ends.  Here: grids, streams, the
context buffer's growth, the argument errors, and sends in / frames out end to end; the
deterministic sets run in tests/test_gpu_txplan_edges.py."""
import ctypes as C

import numpy as np
import pytest

import rxg
import txbuild_opt_ref as oref
import txbuild_ref as ref
import txplan_cases as tc
from test_gpu_txbuild import _peer_tcbs

pytestmark = pytest.mark.gpu

EINVAL = 22


class Bufs:
    """The device side of one call: inputs uploaded, outputs pre-filled (kept until freed)."""

    def __init__(self, eng, c):
        w = tc.expect(c)
        self.eng, self.c, self.w, self.n = eng, c, w, len(c["sends"])
        self.sends = eng.to_device(c["sends"] if self.n else np.zeros(1, rxg.TX_SEND_DTYPE))
        self.so = eng.to_device(c["send_opt"]) if c["send_opt"] is not None and self.n else None
        self.opts = eng.to_device(c["opts"]) if len(c["opts"]) else None
        self.segs = eng.to_device(np.full(len(w["segs"]), tc.FILL, np.uint8))
        self.first = eng.to_device(np.full(len(w["first"]) * 8, tc.FILL, np.uint8))
        self.nxt = eng.to_device(np.full(len(w["next_seq"]) * 4, tc.FILL, np.uint8))
        self.count = eng.to_device(np.full(16, tc.FILL, np.uint8))

    def call(self, eng=None, stream=None):
        c = self.c
        (eng or self.eng).tx_plan_dev(self.sends.ptr, self.n, c["mss"], self.segs.ptr, self.w["cap"], self.first.ptr,
                                      self.count.ptr, send_opt=self.so.ptr if self.so else None,
                                      opts=self.opts.ptr if self.opts else None, nopts=len(c["opts"]),
                                      next_seq=self.nxt.ptr if c["next_seq"] else None, stream=stream)

    def get(self):
        w = self.w
        return dict(segs=self.segs.download(np.uint8, len(w["segs"])), first=self.first.download(np.uint64, len(w["first"])),
                    next_seq=self.nxt.download(np.uint32, len(w["next_seq"])), count=self.count.download(np.uint64, 2))

    def free(self):
        for d in (self.sends, self.so, self.opts, self.segs, self.first, self.nxt, self.count):
            if d is not None:
                d.free()


def compare(got, c, what=""):
    """Every byte of the four buffers against tc.expect(c)."""
    w = tc.expect(c)
    what = f"{c['name']} {what}"
    assert got["count"].tolist() == w["count"].tolist(), what
    if not np.array_equal(got["first"], w["first"]):
        j = int(np.nonzero(got["first"] != w["first"])[0][0])
        raise AssertionError(f"{what}: first[{j}] of {len(c['sends'])} sends: got {int(got['first'][j])} "
                             f"want {int(w['first'][j])}")
    if not np.array_equal(got["next_seq"], w["next_seq"]):
        j = int(np.nonzero(got["next_seq"] != w["next_seq"])[0][0])
        raise AssertionError(f"{what}: next_seq[{j}]: got {int(got['next_seq'][j]):#x} want {int(w['next_seq'][j]):#x}")
    if not np.array_equal(got["segs"], w["segs"]):
        bad = np.nonzero(got["segs"] != w["segs"])[0]
        k, byte = int(bad[0]) // 32, int(bad[0]) % 32
        j = int(np.searchsorted(w["first"][:len(c["sends"]) + 1], k, side="right")) - 1
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first in descriptor {k} (cap {w['cap']}, total "
                             f"{w['total']}; send {j}) byte {byte}: got {int(got['segs'][bad[0]]):#x} "
                             f"want {int(w['segs'][bad[0]]):#x}")


def run(eng, c, what="", stream=None):
    b = Bufs(eng, c)
    try:
        b.call(stream=stream)
        eng.sync()
        got = b.get()
    finally:
        b.free()
    compare(got, c, what)
    return got


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in tc.all_cases()}


@pytest.fixture(scope="module")
def grids(engine):
    """Contexts whose launches are capped at 1 and 2 workgroups, and the occupancy grid."""
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    e1.close()
    e2.close()


# 1. one, two and the occupancy grid's workgroups: the same bytes, the planner's
@pytest.mark.parametrize("name", ["count_513", "count_16385", "lanes_63_64_65", "refused_lanes", "cap_first+1",
                                  "bytes_2^32-1"])
def test_grids_give_identical_bytes(grids, cases, name):
    outs = [run(eng, cases[name], what) for what, eng in grids]
    for o in outs[1:]:
        assert all(np.array_equal(o[k], outs[0][k]) for k in o)


# 2. two calls on two streams of one context, no host wait between them: the second waits on
#    the device for the first one's use of the context's tile sums
def test_two_streams_share_the_context_buffer(engine, cases):
    import torch
    a, b = Bufs(engine, cases["count_16385"]), Bufs(engine, cases["count_16383"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    try:
        for _ in range(3):
            a.call(stream=s1.cuda_stream)
            b.call(stream=s2.cuda_stream)
        engine.stream_sync(s1.cuda_stream)
        engine.stream_sync(s2.cuda_stream)
        compare(a.get(), a.c, "stream 1")
        compare(b.get(), b.c, "stream 2")
    finally:
        a.free()
        b.free()


# 3. a large call after a small one on a fresh context: the buffer grows (after a host wait)
def test_buffer_grows(cases):
    with rxg.Engine(device=0) as eng:
        small, large = Bufs(eng, cases["count_1"]), Bufs(eng, cases["one_segment_sends_2^16+1"])
        try:
            small.call()
            large.call()
            small.call()
            eng.sync()
            compare(small.get(), small.c, "small")
            compare(large.get(), large.c, "large after small")
        finally:
            small.free()
            large.free()


# 4. the -EINVAL list, and nsends == 0
def test_argument_errors_and_no_sends(engine, cases):
    lib = rxg.load_library()
    c = cases["count_65"]
    b = Bufs(engine, c)
    try:
        def call(ctx=engine.ctx, **kw):
            a = dict(sends=b.sends.ptr, nsends=b.n, mss=c["mss"], send_opt=b.so.ptr, opts=b.opts.ptr,
                     nopts=len(c["opts"]), pad=0, segs=b.segs.ptr, cap=b.w["cap"], first=b.first.ptr,
                     next_seq=b.nxt.ptr, count=b.count.ptr)
            a.update(kw)
            return lib.rxg_tx_plan_dev(ctx, C.byref(rxg.DevTxPlan(**a)), None)
        for kw, why in [(dict(sends=None), b"NULL"), (dict(first=None), b"NULL"), (dict(count=None), b"NULL"),
                        (dict(segs=None), b"NULL"), (dict(sends=b.sends.ptr + 4), b"alignment"),
                        (dict(segs=b.segs.ptr + 4), b"alignment"), (dict(first=b.first.ptr + 4), b"alignment"),
                        (dict(count=b.count.ptr + 4), b"alignment"), (dict(opts=b.opts.ptr + 8), b"alignment"),
                        (dict(next_seq=b.nxt.ptr + 2), b"alignment"), (dict(send_opt=b.so.ptr + 2), b"alignment"),
                        (dict(mss=0), b"mss"), (dict(mss=rxg.TX_MAX_DATA + 1), b"mss"),
                        (dict(opts=None), b"opts")]:
            assert call(**kw) == -EINVAL, kw
            err = lib.rxg_last_error()
            assert why in err and b"rxg_tx_plan_dev" in err, (kw, err)
        assert lib.rxg_tx_plan_dev(engine.ctx, None, None) == -EINVAL
        assert call(ctx=None) == -EINVAL
        engine.sync()
        got = b.get()  # nothing was launched: every buffer keeps its fill
        assert all((v.view(np.uint8) == tc.FILL).all() for v in got.values())
        # nsends == 0: count = {0, 0} and first[0] = 0, nothing else
        assert call(nsends=0, segs=None, cap=0, send_opt=None, opts=None, nopts=0, next_seq=None) == 0
        engine.sync()
        got = b.get()
        assert got["count"].tolist() == [0, 0] and int(got["first"][0]) == 0
        assert (got["first"][1:] == 0xA5A5A5A5A5A5A5A5).all() and (got["next_seq"] == 0xA5A5A5A5).all()
        assert (got["segs"] == tc.FILL).all()
        # not errors: segs NULL with cap 0; opts NULL with nopts 0 (every send that names a block is refused)
        assert call(segs=None, cap=0) == 0
        assert call(opts=None, nopts=0) == 0
        engine.sync()
        assert int(b.count.download(np.uint64, 2)[1]) == int((c["send_opt"] > 0).sum())
    finally:
        b.free()


# 5. the least alignment, checked: the sends from the second on, every output one entry in
def test_least_alignment(engine, cases):
    c = cases["count_257"]
    sub = tc.case("count_257_from_1", c["sends"][1:], send_opt=c["send_opt"][1:])
    w = tc.expect(sub)
    b = Bufs(engine, c)
    try:
        engine.tx_plan_dev(b.sends.ptr + 40, b.n - 1, c["mss"], b.segs.ptr + 32 + 8, w["cap"], b.first.ptr + 8,
                           b.count.ptr, send_opt=b.so.ptr + 4, opts=b.opts.ptr, nopts=len(c["opts"]),
                           next_seq=b.nxt.ptr + 4)
        engine.sync()
        segs = b.segs.download(np.uint8, len(tc.expect(c)["segs"]))
        assert (segs[:40] == tc.FILL).all()
        assert np.array_equal(segs[40:40 + w["total"] * 32], w["segs"][:w["total"] * 32])
        assert (segs[40 + w["total"] * 32:] == tc.FILL).all()
        first = b.first.download(np.uint64, b.n + 1)
        assert int(first[0]) == 0xA5A5A5A5A5A5A5A5 and np.array_equal(first[1:], w["first"][:b.n])
        nxt = b.nxt.download(np.uint32, b.n)
        assert int(nxt[0]) == 0xA5A5A5A5 and np.array_equal(nxt[1:], w["next_seq"][:b.n - 1])
    finally:
        b.free()


# 6. sends in, frames out: rxg_tx_plan_dev, then rxg_tx_build_opt_dev with n = rxg_tx_plan_count
def test_end_to_end_sends_in_frames_out(engine):
    r = np.random.default_rng(37)
    flows = ref.make_flows(8)
    table = np.array([rxg.tx_opt_timestamp(0x01020304, 0x0A0B0C0D), rxg.tx_opt_ref_ack(), rxg.tx_opt_set(b"")],
                     dtype=rxg.TX_OPT_DTYPE)
    nb = np.concatenate([[0, 1, 1447, 1448, 1449, 1460, 1461, 20000], r.integers(0, 6000, 29)])
    assert len(nb) == 37
    payload = r.integers(0, 256, int(nb.sum()) + 16, dtype=np.uint8)
    sends = tc.make_sends(nb, 37, flags=r.choice([tc.ACK, tc.ACK | tc.PSH, tc.ACK | tc.FIN, tc.SYN], 37),
                          src_off=np.concatenate([[0], np.cumsum(nb)[:-1]]).astype(np.uint64))
    sends["flow"] = r.integers(0, len(flows), 37)
    so = r.integers(0, len(table) + 1, 37).astype(np.uint32)
    assert set(so.tolist()) == {0, 1, 2, 3}
    n = rxg.tx_plan_count(sends, tc.MSS, so, table)
    h_segs, h_next = rxg.tx_plan_opt(sends, tc.MSS, so, table)
    assert n == len(h_segs) > 37
    stride64 = (54 + 40 + tc.MSS + 63) // 64
    want_arena, want_len, want_stats = engine.tx_build(payload, flows, h_segs, slot0=0, stride64=stride64, opts=table)
    assert list(want_stats) == [n, 0]
    pad = np.zeros((len(payload) + 15) // 16 * 16, np.uint8)
    pad[:len(payload)] = payload
    ds, dso, dopt = engine.to_device(sends), engine.to_device(so), engine.to_device(table)
    dsegs, dfirst = engine.to_device(np.full(n * 32, tc.FILL, np.uint8)), engine.alloc(38 * 8)
    dnext, dcount = engine.alloc(37 * 4), engine.alloc(16)
    dp, df = engine.to_device(pad), engine.to_device(flows)
    da, dl, dst = engine.to_device(np.zeros(len(want_arena), np.uint8)), engine.alloc(n * 2), engine.to_device(
        np.zeros(2, np.uint64))
    try:
        # no host wait between the plan and the build: n comes from the host count
        engine.tx_plan_dev(ds.ptr, 37, tc.MSS, dsegs.ptr, n, dfirst.ptr, dcount.ptr, send_opt=dso.ptr, opts=dopt.ptr,
                           nopts=len(table), next_seq=dnext.ptr)
        engine.tx_build_opt_dev(dp.ptr, len(payload), df.ptr, len(flows), dsegs.ptr, n, da.ptr, dl.ptr, dopt.ptr,
                                len(table), None, 0, stride64, dst.ptr)
        engine.sync()
        assert dcount.download(np.uint64, 2).tolist() == [n, 0]
        assert dsegs.download(np.uint8, n * 32).tobytes() == h_segs.tobytes()
        assert np.array_equal(dnext.download(np.uint32, 37), h_next)
        arena, lens = da.download(np.uint8, len(want_arena)), dl.download(np.uint16, n)
        assert dst.download(np.uint64, 2).tolist() == [n, 0]
        assert np.array_equal(lens, want_len) and np.array_equal(arena, want_arena)
    finally:
        for d in (ds, dso, dopt, dsegs, dfirst, dnext, dcount, dp, df, da, dl, dst):
            d.free()
    # the frames are the model's, and verify to checksum 0 through the receive path
    off = (np.arange(n) * stride64).astype(np.uint32)
    model, mlen, _ = oref.build(payload, flows, h_segs, table, off, n * stride64)
    assert np.array_equal(lens, mlen) and np.array_equal(arena[:n * stride64 * 64], model)
    with rxg.Engine(device=0) as peer:
        peer.tcb_load(_peer_tcbs(flows), np.ones(len(flows), np.uint8))
        recs = peer.rx_arena(arena, off, lens, rxg.REC48)
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert (recs["c"]["flags"] & (rxg.F_IP_OK | rxg.F_TCP_OK) == rxg.F_IP_OK | rxg.F_TCP_OK).all()
    assert np.array_equal(recs["seq"], h_segs["seq"]) and np.array_equal(recs["c"]["datalen"], h_segs["data_len"])
