"""GPU: rxg_tx_build_dev (headers, payload and both checksums of a batch of TCP segments in
one pass) against the reference model tests/txbuild_ref.py -- a restatement of sendtcpdata /
ip_out / ether_out with the oracle's checksums, itself pinned in tests/test_txbuild_host.py --
never against the kernel's own output.  Every frame pool is pre-filled with 0xA5 and compared
whole, so a stray write anywhere in it fails the comparison."""
import ctypes as C

import numpy as np
import pytest

import rxg
import txbuild_ref as ref

pytestmark = pytest.mark.gpu

FILL = 0xA5
EINVAL = 22


def run(eng, payload, flows, segs, nslots, off64=None, slot0=0, stride64=0, nflows=None, payload_bytes=None,
        stats0=(0, 0)):
    """One rxg_tx_build_dev over a pool of nslots slots holding FILL: (pool, len, stats)."""
    n = len(segs)
    pad = np.zeros((len(payload) + 15) // 16 * 16 or 16, np.uint8)
    pad[:len(payload)] = payload
    dp, df, ds = eng.to_device(pad), eng.to_device(flows), eng.to_device(segs)
    do = eng.to_device(np.ascontiguousarray(off64, dtype=np.uint32)) if off64 is not None else None
    da = eng.to_device(np.full(nslots * 64, FILL, np.uint8))
    dl = eng.to_device(np.full(n, 0xBEEF, np.uint16))
    dst = eng.to_device(np.array(stats0, dtype=np.uint64))
    try:
        eng.tx_build_dev(dp.ptr, len(payload) if payload_bytes is None else payload_bytes, df.ptr,
                         len(flows) if nflows is None else nflows, ds.ptr, n, da.ptr, dl.ptr,
                         do.ptr if do else None, slot0, stride64, dst.ptr)
        eng.sync()
        return da.download(np.uint8, nslots * 64), dl.download(np.uint16, n), dst.download(np.uint64, 2)
    finally:
        for d in (dp, df, ds, do, da, dl, dst):
            if d is not None:
                d.free()


def explain(got, want, off64, lens):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return ""
    b = int(bad[0])
    starts = np.asarray(off64, dtype=np.int64) * 64
    i = int(np.argmax((starts <= b) & (b < starts + (np.asarray(lens, dtype=np.int64) + 54 + 63) // 64 * 64)))
    return f"{len(bad)} bytes differ, first at pool byte {b}: frame {i} (data_len {int(lens[i])}) byte {b - int(starts[i])}, " \
           f"got {int(got[b]):#x} want {int(want[b]):#x}"


@pytest.fixture(scope="module")
def flows():
    return ref.make_flows(8)


@pytest.fixture(scope="module")
def payload():
    return np.random.default_rng(11).integers(0, 256, 1 << 17, dtype=np.uint8)


# 1. every length x every source alignment, byte-exact (the pool compared whole: also 4.)
def test_lengths_and_alignments_byte_exact(engine, flows, payload):
    lens = np.repeat(ref.LENGTHS, 16)
    r = np.random.default_rng(1)
    base = r.integers(0, (len(payload) - 65481 - 16) // 16, len(lens)) * 16
    segs = ref.make_segs(lens, base + np.tile(np.arange(16), len(ref.LENGTHS)), len(flows), seed=2)
    assert sorted(set(int(x) % 16 for x in segs["src_off"][:16])) == list(range(16))
    off, nslots = ref.packed_offsets(lens, r.permutation(len(lens)))
    want, wlen, wstats = ref.build(payload, flows, segs, off, nslots + 2, fill=FILL)
    got, glen, gstats = run(engine, payload, flows, segs, nslots + 2, off64=off)
    assert np.array_equal(glen, wlen)
    assert np.array_equal(got, want), explain(got, want, off, lens)
    assert list(gstats) == list(wstats) == [len(lens), 0]


# 2. wave and workgroup edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_wave_and_workgroup_edges(engine, flows, payload, n):
    r = np.random.default_rng(100 + n)
    lens = r.choice(ref.LENGTHS, n)
    segs = ref.make_segs(lens, r.integers(0, len(payload) - 65481, n), len(flows), seed=n)
    off, nslots = ref.packed_offsets(lens, r.permutation(n))
    want, wlen, wstats = ref.build(payload, flows, segs, off, nslots + 1, fill=FILL)
    got, glen, gstats = run(engine, payload, flows, segs, nslots + 1, off64=off, stats0=(5, 7))
    assert np.array_equal(glen, wlen)
    assert np.array_equal(got, want), explain(got, want, off, lens)
    assert list(gstats) == [5 + n, 7]  # added to, not overwritten


# 3. fixed stride == the same offsets as a list
@pytest.mark.parametrize("stride64,maxlen", [(1, 10), (24, 1461), (1024, 65481)])
def test_strided_equals_list(engine, flows, payload, stride64, maxlen):
    r = np.random.default_rng(stride64)
    n, slot0 = 200, 3
    lens = r.choice([x for x in ref.LENGTHS if x <= maxlen], n)
    segs = ref.make_segs(lens, r.integers(0, len(payload) - 65481, n), len(flows), seed=9)
    off = (slot0 + np.arange(n) * stride64).astype(np.uint32)
    nslots = int(off[-1]) + stride64
    want, wlen, _ = ref.build(payload, flows, segs, off, nslots, fill=FILL)
    got_s, len_s, st_s = run(engine, payload, flows, segs, nslots, slot0=slot0, stride64=stride64)
    got_l, len_l, st_l = run(engine, payload, flows, segs, nslots, off64=off)
    assert np.array_equal(got_s, got_l) and np.array_equal(len_s, len_l) and list(st_s) == list(st_l) == [n, 0]
    assert np.array_equal(len_s, wlen)
    assert np.array_equal(got_s, want), explain(got_s, want, off, lens)


# 4. no stray writes, stated on its own: outside the built frames' lines the pool keeps its
# fill, inside them the bytes at or past len are zero
def test_no_stray_writes(engine, flows, payload):
    r = np.random.default_rng(5)
    n = 300
    lens = r.choice(ref.LENGTHS[:-2], n)
    segs = ref.make_segs(lens, r.integers(0, len(payload) - 65481, n), len(flows), seed=6)
    # frames spread over the pool with untouched slots between them
    sl = ref.slots_of(lens)
    off = (np.cumsum(sl + r.integers(0, 3, n)) - sl + 1).astype(np.uint32)
    nslots = int(off[-1] + sl[-1]) + 4
    got, glen, _ = run(engine, payload, flows, segs, nslots, off64=off)
    inside = np.zeros(nslots * 64, dtype=bool)
    for o, ln in zip(off, glen):
        a, end = int(o) * 64, int(o) * 64 + (int(ln) + 63) // 64 * 64
        inside[a:end] = True
        assert not got[a + int(ln):end].any()
    assert (glen == 54 + lens).all()
    assert (got[~inside] == FILL).all()


# 5. skipped segments: never followed, counted, their slots untouched
def test_skipped_segments(engine, payload):
    flows = ref.make_flows(9)  # one entry more than the bound passed
    nflows, pbytes = 8, 40000  # and 64 KiB of payload past the bound passed
    r = np.random.default_rng(8)
    n = 150
    lens = r.choice(ref.LENGTHS[:-1], n)
    so = r.integers(0, pbytes - 8960, n)
    segs = ref.make_segs(lens, so, nflows, seed=12)
    bad_flow, bad_len, bad_off = [3, 64, 149], [0, 70, 128], [5, 63, 100, 140]
    segs["flow"][bad_flow] = nflows
    segs["data_len"][bad_len] = rxg.TX_MAX_DATA + 1
    for i in bad_off:
        segs["src_off"][i] = pbytes + 1 - int(segs["data_len"][i])
    edge = [7, 90]  # src_off + data_len == payload_bytes exactly: built
    for i in edge:
        segs["src_off"][i] = pbytes - int(segs["data_len"][i])
    off = (np.arange(n) * 141).astype(np.uint32)  # 141 slots: a frame of 8960 bytes
    nslots = n * 141 + 1024
    want, wlen, wstats = ref.build(payload[:pbytes], flows[:nflows], segs, off, nslots, fill=FILL)
    skipped = sorted(bad_flow + bad_len + bad_off)
    assert sorted(np.nonzero(wlen == 0)[0]) == skipped and list(wstats) == [n - len(skipped), len(skipped)]
    assert len(payload) >= pbytes + (64 << 10)
    got, glen, gstats = run(engine, payload, flows, segs, nslots, off64=off, nflows=nflows, payload_bytes=pbytes)
    assert sorted(np.nonzero(glen == 0)[0]) == skipped
    assert np.array_equal(glen, wlen) and list(gstats) == list(wstats)
    for i in skipped:
        assert (got[int(off[i]) * 64:(int(off[i]) + 141) * 64] == FILL).all(), i
    assert np.array_equal(got, want), explain(got, want, off, segs["data_len"])


def _peer_tcbs(flows):
    """The peers' TCBs for our flows: our segment's dst_port / dst_addr are theirs."""
    t = np.zeros(len(flows), dtype=rxg.TCB_DTYPE)
    t["dport"], t["sport"] = flows["sport"], flows["dport"]
    t["ipv4_dst"] = flows["ipv4_src"].byteswap()
    t["ipv4_src"] = flows["ipv4_dst"].byteswap()
    t["state"] = rxg.TCP_ESTABLISHED
    t["identifier"] = 1 + np.arange(len(flows))
    return t


# 6. + 7. the built frames through the shipped receive path and the shipped tx checksum
def test_round_trip_rx_and_tx_cksum(engine, flows, payload):
    r = np.random.default_rng(21)
    n = 400
    lens = r.choice(ref.LENGTHS, n)
    segs = ref.make_segs(lens, r.integers(0, len(payload) - 65481, n), len(flows), seed=22)
    off, nslots = ref.packed_offsets(lens)
    pool, flen, _ = run(engine, payload, flows, segs, nslots, off64=off)
    # (a context of its own for the peers' table: the session engine's mirror stays as it is)
    with rxg.Engine(device=0) as peer:
        peer.tcb_load(_peer_tcbs(flows), np.ones(len(flows), np.uint8))
        recs = peer.rx_arena(pool, off, flen, rxg.REC48)
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all()
    assert (recs["c"]["flags"] & (rxg.F_IP_OK | rxg.F_TCP_OK) == rxg.F_IP_OK | rxg.F_TCP_OK).all()
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert np.array_equal(recs["c"]["tcb_idx"], segs["flow"].astype(np.int32))
    assert np.array_equal(recs["c"]["datalen"], lens.astype(np.int32))
    assert np.array_equal(recs["seq"], segs["seq"]) and np.array_equal(recs["ack"], segs["ack"])
    # the fused checksums are the ones rxg_tx_cksum_dev writes: it changes no byte
    again = engine.tx_arena(pool, off, flen)
    assert np.array_equal(again, pool)


# 8. plan -> build of one 1 MiB send
def test_plan_then_build_one_mebibyte(engine, flows):
    data = np.random.default_rng(31).integers(0, 256, 1 << 20, dtype=np.uint8)
    mss = 1460
    segs, nxt = rxg.tx_plan([(5, 0xFFFF0000, 99, 0, len(data), rxg.TCP_FLAG_ACK | rxg.TCP_FLAG_PSH, 0xFFFF, 0xFFF0)], mss)
    n = len(segs)
    assert n == -(-len(data) // mss)
    arena, lens, stats = engine.tx_build(data, flows, segs, slot0=0, stride64=24)
    assert list(stats) == [n, 0]
    frames = arena.reshape(-1, 24 * 64)
    got = np.concatenate([frames[i, 54:int(lens[i])] for i in range(n)])
    assert np.array_equal(got, data)
    seqs = frames[:, 38:42].copy().view(">u4").ravel().astype(np.uint64)
    assert np.array_equal(seqs, segs["seq"])
    assert np.array_equal((seqs[1:] - seqs[:-1]) & 0xFFFFFFFF, (lens[:-1] - 54).astype(np.uint64))
    assert int(nxt[0]) == (0xFFFF0000 + len(data)) & 0xFFFFFFFF
    assert (frames[:-1, 47] == rxg.TCP_FLAG_ACK).all() and frames[-1, 47] == rxg.TCP_FLAG_ACK | rxg.TCP_FLAG_PSH
    want, _, _ = ref.build(data, flows, segs, np.arange(n) * 24, n * 24)
    assert np.array_equal(arena[:n * 24 * 64], want)


# 9. argument errors, and n == 0
def test_argument_errors(engine, flows, payload):
    lib = rxg.load_library()
    segs = ref.make_segs(np.array([100, 200]), np.array([0, 300]), len(flows), seed=1)
    dp, df, ds = engine.to_device(payload[:4096]), engine.to_device(flows), engine.to_device(segs)
    da, dl, dst = engine.alloc(64 * 64), engine.alloc(16), engine.alloc(32)
    do = engine.to_device(np.array([0, 8, 0, 0], np.uint32))
    try:
        def call(**kw):
            a = dict(payload=dp.ptr, payload_bytes=4096, flows=df.ptr, nflows=len(flows), n=2, segs=ds.ptr,
                     frames=da.ptr, off64=do.ptr, slot0=0, stride64=0, len=dl.ptr, stats=dst.ptr)
            a.update(kw)
            b = rxg.DevTxBuild(**a)
            return lib.rxg_tx_build_dev(engine.ctx, C.byref(b), None)
        assert call() == 0
        engine.sync()
        for kw, why in [(dict(frames=da.ptr + 16), b"alignment"), (dict(frames=da.ptr + 32), b"alignment"),
                        (dict(segs=ds.ptr + 4), b"alignment"), (dict(flows=df.ptr + 4), b"alignment"),
                        (dict(off64=do.ptr + 2), b"alignment"), (dict(len=dl.ptr + 1), b"alignment"),
                        (dict(stats=dst.ptr + 4), b"alignment"), (dict(payload=dp.ptr + 8), b"alignment"),
                        (dict(off64=None, stride64=0), b"stride64"),
                        (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
                        (dict(off64=None, slot0=0, stride64=0xFFFFFFFF, n=3), b"2^32"),
                        (dict(frames=None), b"NULL"), (dict(segs=None), b"NULL"), (dict(flows=None), b"NULL"),
                        (dict(len=None), b"NULL"), (dict(payload=None), b"NULL")]:
            assert call(**kw) == -EINVAL, kw
            assert why in lib.rxg_last_error(), (kw, lib.rxg_last_error())
        assert lib.rxg_tx_build_dev(engine.ctx, None, None) == -EINVAL
        # n == 0 does nothing, whatever else is set; stats may be NULL
        assert call(n=0, frames=None, segs=None) == 0
        assert call(stats=None) == 0
        assert call(off64=None, slot0=0, stride64=8) == 0
        engine.sync()
    finally:
        for d in (dp, df, ds, da, dl, dst, do):
            d.free()
