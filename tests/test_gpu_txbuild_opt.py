"""GPU: rxg_tx_build_opt_dev (rxg_tx_build_dev for segments that carry a TCP option block)
against the model tests/txbuild_opt_ref.py -- txbuild_ref's frame extended by the block, with
the oracle's checksums, pinned in tests/test_txbuild_opt_host.py -- never against the kernel's
own output.  As in test_gpu_txbuild.py every frame pool is pre-filled with 0xA5 and compared
whole, so a stray write anywhere in it fails the comparison.  Every block holds garbage in
what the call must ignore (bytes[] at and past len, the reserved fields)."""
import ctypes as C

import numpy as np
import pytest

import rxg
import txbuild_opt_ref as oref
import txbuild_ref as ref
from test_gpu_txbuild import FILL, _peer_tcbs, run

pytestmark = pytest.mark.gpu

EINVAL = 22
HDR = 54


def run_opt(eng, payload, flows, segs, opts, nslots, off64=None, slot0=0, stride64=0, nflows=None, payload_bytes=None,
            nopts=None, stats0=(0, 0)):
    """One rxg_tx_build_opt_dev over a pool of nslots slots holding FILL: (pool, len, stats)."""
    n = len(segs)
    pad = np.zeros((len(payload) + 15) // 16 * 16 or 16, np.uint8)
    pad[:len(payload)] = payload
    dp, df, ds = eng.to_device(pad), eng.to_device(flows), eng.to_device(segs)
    dopt = eng.to_device(opts) if len(opts) else None
    do = eng.to_device(np.ascontiguousarray(off64, dtype=np.uint32)) if off64 is not None else None
    da = eng.to_device(np.full(nslots * 64, FILL, np.uint8))
    dl = eng.to_device(np.full(n, 0xBEEF, np.uint16))
    dst = eng.to_device(np.array(stats0, dtype=np.uint64))
    try:
        eng.tx_build_opt_dev(dp.ptr, len(payload) if payload_bytes is None else payload_bytes, df.ptr,
                             len(flows) if nflows is None else nflows, ds.ptr, n, da.ptr, dl.ptr,
                             dopt.ptr if dopt else None, len(opts) if nopts is None else nopts,
                             do.ptr if do else None, slot0, stride64, dst.ptr)
        eng.sync()
        return da.download(np.uint8, nslots * 64), dl.download(np.uint16, n), dst.download(np.uint64, 2)
    finally:
        for d in (dp, df, ds, dopt, do, da, dl, dst):
            if d is not None:
                d.free()


def explain(got, want, off64, flens, segs):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return ""
    b = int(bad[0])
    starts = np.asarray(off64, dtype=np.int64) * 64
    i = int(np.argmax((starts <= b) & (b < starts + (np.asarray(flens, dtype=np.int64) + 63) // 64 * 64)))
    return f"{len(bad)} bytes differ, first at pool byte {b}: frame {i} (data_len {int(segs[i]['data_len'])}, " \
           f"block {int(segs[i]['reserved'])}, src_off {int(segs[i]['src_off'])}) byte {b - int(starts[i])}, " \
           f"got {int(got[b]):#x} want {int(want[b]):#x}"


def check(eng, payload, flows, segs, opts, off, nslots, what="", model=None, **kw):
    """One build on `eng` against the model's: len, the whole pool, stats.  Returns the pool."""
    stats0 = kw.get("stats0", (0, 0))
    pbytes = kw.get("payload_bytes", len(payload))
    nflows = kw.get("nflows", len(flows))
    nopts = kw.get("nopts", len(opts))
    want, wlen, wstats = model or oref.build(payload[:pbytes], flows[:nflows], segs, opts, off, nslots, fill=FILL,
                                             nopts=nopts)
    got, glen, gstats = run_opt(eng, payload, flows, segs, opts, nslots, off64=off, **kw)
    assert np.array_equal(glen, wlen), what
    assert np.array_equal(got, want), what + " " + explain(got, want, off, wlen, segs)
    assert [int(x) for x in gstats] == [int(wstats[0]) + stats0[0], int(wstats[1]) + stats0[1]], what
    return got


@pytest.fixture(scope="module")
def flows():
    return ref.make_flows(8)


@pytest.fixture(scope="module")
def payload():
    return np.random.default_rng(11).integers(0, 256, 1 << 17, dtype=np.uint8)


@pytest.fixture(scope="module")
def opts():
    """Blocks 1..7: lengths 0, 4, 8, 12, 16, 28, 40 (block k has OPT_LENS[k - 1] bytes)."""
    return oref.make_opts(oref.OPT_LENS)


LONG_ALIGN = [0, 5, 6, 11, 15]


def cases_for(O):
    """(data_len, src_off mod 16): every alignment on the lengths up to 300, five on the longer
    ones, RXG_TX_MAX_DATA - O once."""
    out = []
    for L in oref.payload_lengths(O):
        out += [(L, a) for a in (range(16) if L <= 300 else LONG_ALIGN)]
    return out + [(rxg.TX_MAX_DATA - O, 9)]


# 1. every option length x the payload lengths at its edges x source alignment, byte-exact
@pytest.mark.parametrize("k", range(1, len(oref.OPT_LENS) + 1))
def test_option_lengths_and_alignments_byte_exact(engine, flows, payload, opts, k):
    O = int(opts[k - 1]["len"])
    cs = cases_for(O)
    dl = np.array([c[0] for c in cs])
    r = np.random.default_rng(200 + O)
    base = r.integers(0, (len(payload) - rxg.TX_MAX_DATA - 16) // 16, len(cs)) * 16
    segs = ref.make_segs(dl, base + np.array([c[1] for c in cs]), len(flows), seed=300 + O)
    segs["reserved"] = k
    if O == 0:  # half of them without a block at all
        segs["reserved"][::2] = 0
    for L in (0, 1, 2, 256 - HDR - O, 256 - HDR - O + 1):
        assert sorted(int(s) % 16 for s in segs["src_off"][dl == L]) == list(range(16)), L
    off, nslots = oref.packed_offsets(dl, np.full(len(cs), O), r.permutation(len(cs)))
    check(engine, payload, flows, segs, opts, off, nslots + 2)


# 2. segments of several O and of none in the same 64-descriptor slice
def mixed_case(n, payload, flows, opts, seed, max_len=2731):
    r = np.random.default_rng(seed)
    kk = r.integers(0, len(opts) + 1, n)
    ol = np.array([int(opts[k - 1]["len"]) if k else 0 for k in kk])
    dl = np.array([int(r.choice([x for x in oref.payload_lengths(int(o)) if x <= max_len])) for o in ol])
    if n >= 64:  # one size class, every H: a frame of exactly two lines without a block and with each block
        kk[:len(opts) + 1] = np.arange(len(opts) + 1)
        ol[:len(opts) + 1] = [0] + [int(x) for x in opts["len"]]
        dl[:len(opts) + 1] = 128 - HDR - ol[:len(opts) + 1]
    segs = ref.make_segs(dl, r.integers(0, len(payload) - max_len, n), len(flows), seed=seed + 1)
    segs["reserved"] = kk
    off, nslots = oref.packed_offsets(dl, ol, r.permutation(n))
    return segs, dl, ol, off, nslots


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_mixed_slices(engine, flows, payload, opts, n):
    segs, dl, ol, off, nslots = mixed_case(n, payload, flows, opts, seed=400 + n)
    if n >= 64:  # one size class holds different H: frames of 2 lines with every O and with no block
        two = [i for i in range(64) if 64 < HDR + ol[i] + dl[i] <= 128]
        assert {int(ol[i]) for i in two} == set(oref.OPT_LENS)
        assert set(segs["reserved"][:64].tolist()) == set(range(len(opts) + 1))
    check(engine, payload, flows, segs, opts, off, nslots + 1, stats0=(5, 7))


# 3. reserved == 0 everywhere: rxg_tx_build_dev's pool, len and stats, and the old model's
def test_reserved_zero_equals_tx_build_dev(engine, flows, payload, opts):
    lens = np.repeat(ref.CLASS_LENGTHS + [8960], 4)
    r = np.random.default_rng(31)
    segs = ref.make_segs(lens, r.integers(0, len(payload) - 8960, len(lens)), len(flows), seed=32)
    segs["flow"][5] = len(flows)  # a skipped one
    off, nslots = ref.packed_offsets(lens, r.permutation(len(lens)))
    want, wlen, wstats = ref.build(payload, flows, segs, off, nslots + 1, fill=FILL)
    old = run(engine, payload, flows, segs, nslots + 1, off64=off)
    new = run_opt(engine, payload, flows, segs, opts, nslots + 1, off64=off)
    none = run_opt(engine, payload, flows, segs, opts[:0], nslots + 1, off64=off)  # opts NULL, nopts 0
    for got in (old, new, none):
        assert np.array_equal(got[1], wlen) and np.array_equal(got[0], want)
        assert list(got[2]) == list(wstats) == [len(lens) - 1, 1]


# 4. unchanged behaviour (passes without the feature): rxg_tx_build_dev ignores `reserved`
def test_tx_build_dev_ignores_reserved(engine, flows, payload):
    r = np.random.default_rng(41)
    lens = r.choice(ref.CLASS_LENGTHS, 200)
    segs = ref.make_segs(lens, r.integers(0, len(payload) - 2731, 200), len(flows), seed=42)
    off, nslots = ref.packed_offsets(lens)
    plain = run(engine, payload, flows, segs, nslots, off64=off)
    segs["reserved"] = r.integers(1, 1 << 32, 200, dtype=np.uint64)
    marked = run(engine, payload, flows, segs, nslots, off64=off)
    want, wlen, wstats = ref.build(payload, flows, segs, off, nslots, fill=FILL)
    for got in (plain, marked):
        assert np.array_equal(got[0], want) and np.array_equal(got[1], wlen) and list(got[2]) == list(wstats)


# 5. skipped segments: never followed, counted, their slots untouched
def test_skipped_segments(engine, flows, payload):
    table = oref.make_opts([12, 44, 6, 40, 28, 16])  # one entry more than the bound passed
    nopts = 5
    r = np.random.default_rng(51)
    n = 160
    kk = r.choice([0, 1, 4, 5], n)
    dl = r.choice([0, 1, 9, 10, 11, 100, 139, 1000, 1460], n)
    segs = ref.make_segs(dl, r.integers(0, len(payload) - rxg.TX_MAX_DATA, n), len(flows), seed=52)
    segs["reserved"] = kk
    past, long_len, odd_len = [3, 64, 159], [10, 70], [20, 129]
    too_much = {7: 1, 90: 4, 140: 0}  # data_len == RXG_TX_MAX_DATA - O + 1 with block k
    ok_edge = {8: 1, 91: 4}           # data_len == RXG_TX_MAX_DATA - O: built
    segs["reserved"][past] = nopts + 1            # a block that is there, beyond the bound passed
    segs["reserved"][long_len] = 2                # len 44
    segs["reserved"][odd_len] = 3                 # len 6
    segs["reserved"][[11, 12]] = [0xFFFFFFFF, 1 << 31]
    tlen = [0, 12, 44, 6, 40, 28]
    for i, k in too_much.items():
        segs["reserved"][i], segs["data_len"][i] = k, rxg.TX_MAX_DATA - tlen[k] + 1
    for i, k in ok_edge.items():
        segs["reserved"][i], segs["data_len"][i], segs["src_off"][i] = k, rxg.TX_MAX_DATA - tlen[k], 3
    off = (np.arange(n) * 1024).astype(np.uint32)
    nslots = n * 1024
    want, wlen, wstats = oref.build(payload, flows, segs, table, off, nslots, fill=FILL, nopts=nopts)
    skipped = sorted(past + long_len + odd_len + [11, 12] + [i for i in too_much if i != 140] + [140])
    assert sorted(np.nonzero(wlen == 0)[0]) == skipped and list(wstats) == [n - len(skipped), len(skipped)]
    assert all(int(wlen[i]) == 65535 for i in ok_edge)
    got, glen, gstats = run_opt(engine, payload, flows, segs, table, nslots, off64=off, nopts=nopts)
    assert sorted(np.nonzero(glen == 0)[0]) == skipped
    assert np.array_equal(glen, wlen) and list(gstats) == list(wstats)
    for i in skipped:
        assert (got[int(off[i]) * 64:(int(off[i]) + 1024) * 64] == FILL).all(), i
    assert np.array_equal(got, want), explain(got, want, off, wlen, segs)


# 6. fixed stride == the same offsets as a list
def test_strided_equals_list(engine, flows, payload, opts):
    n, slot0, stride64 = 200, 3, 25
    segs, dl, ol, _, _ = mixed_case(n, payload, flows, opts, seed=61, max_len=1461)
    assert int((HDR + ol + dl).max()) <= stride64 * 64  # (1443 bytes behind 40 option bytes: 25 lines)
    off = (slot0 + np.arange(n) * stride64).astype(np.uint32)
    nslots = int(off[-1]) + stride64
    want, wlen, _ = oref.build(payload, flows, segs, opts, off, nslots, fill=FILL)
    got_s, len_s, st_s = run_opt(engine, payload, flows, segs, opts, nslots, slot0=slot0, stride64=stride64)
    got_l, len_l, st_l = run_opt(engine, payload, flows, segs, opts, nslots, off64=off)
    assert np.array_equal(got_s, got_l) and np.array_equal(len_s, len_l) and list(st_s) == list(st_l) == [n, 0]
    assert np.array_equal(len_s, wlen)
    assert np.array_equal(got_s, want), explain(got_s, want, off, wlen, segs)


# 7. a grid of one workgroup: its waves take several slices each, the same bytes
def test_capped_grid(engine, flows, payload, opts):
    n = 64 * 4 * 2 + 37
    segs, dl, ol, off, nslots = mixed_case(n, payload, flows, opts, seed=71)
    segs["reserved"][[5, 300]] = len(opts) + 1
    model = oref.build(payload, flows, segs, opts, off, nslots + 1, fill=FILL)
    assert list(model[2]) == [n - 2, 2]
    with rxg.Engine(device=0, max_blocks=1) as one:
        a = check(one, payload, flows, segs, opts, off, nslots + 1, "max_blocks 1", model)
    b = check(engine, payload, flows, segs, opts, off, nslots + 1, "occupancy grid", model)
    assert np.array_equal(a, b)


# 8. the built frames through the shipped receive path and the shipped tx checksum
def test_round_trip_rx_and_tx_cksum(engine, flows, payload, opts):
    n = 400
    segs, dl, ol, off, nslots = mixed_case(n, payload, flows, opts, seed=81)
    pool, flen, stats = run_opt(engine, payload, flows, segs, opts, nslots, off64=off)
    assert list(stats) == [n, 0] and np.array_equal(flen, oref.frame_lens(dl, ol))
    with rxg.Engine(device=0) as peer:
        peer.tcb_load(_peer_tcbs(flows), np.ones(len(flows), np.uint8))
        recs = peer.rx_arena(pool, off, flen, rxg.REC48)
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all()
    assert (recs["c"]["flags"] & (rxg.F_IP_OK | rxg.F_TCP_OK) == rxg.F_IP_OK | rxg.F_TCP_OK).all()
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert np.array_equal(recs["c"]["tcb_idx"], segs["flow"].astype(np.int32))
    assert np.array_equal(recs["c"]["datalen"], dl.astype(np.int32))
    assert np.array_equal(recs["data_off"], ((5 + ol // 4) << 4).astype(np.uint8))
    assert np.array_equal(recs["seq"], segs["seq"]) and np.array_equal(recs["ack"], segs["ack"])
    again = engine.tx_arena(pool, off, flen)
    assert np.array_equal(again, pool)


# 9. plan -> build through the binding: a send with the timestamp block, and the reference's ACK
def test_plan_then_build_with_timestamps_and_sendack(engine, flows):
    data = np.random.default_rng(91).integers(0, 256, 100000, dtype=np.uint8)
    table = np.array([rxg.tx_opt_timestamp(0x11223344, 0x55667788), rxg.tx_opt_ref_ack()], dtype=rxg.TX_OPT_DTYPE)
    sends = [(5, 0xFFFF0000, 99, 0, len(data), rxg.TCP_FLAG_ACK | rxg.TCP_FLAG_PSH, 0xFFFF, 0xFFF0),
             (2, 7, 8, 0, 0, rxg.TCP_FLAG_ACK, 12000, 1)]  # sendack: no data, rx_win 12000 raw
    segs, nxt = rxg.tx_plan_opt(sends, 1460, [1, 2], table)
    n = len(segs)
    assert n == -(-len(data) // 1448) + 1 and int(nxt[0]) == (0xFFFF0000 + len(data)) & 0xFFFFFFFF
    arena, lens, stats = engine.tx_build(data, flows, segs, slot0=0, stride64=24, opts=table)
    assert list(stats) == [n, 0]
    frames = arena[:n * 24 * 64].reshape(n, 24 * 64)
    assert np.array_equal(np.concatenate([frames[i, 66:int(lens[i])] for i in range(n - 1)]), data)
    assert (frames[:-1, 46] == 0x80).all() and frames[-1, 46] == 0xA0 and int(lens[-1]) == 74
    want, wlen, _ = oref.build(data, flows, segs, table, np.arange(n) * 24, n * 24)
    assert np.array_equal(lens, wlen) and np.array_equal(arena[:n * 24 * 64], want)


# 10. argument errors, and n == 0
def test_argument_errors(engine, flows, payload, opts):
    lib = rxg.load_library()
    segs = ref.make_segs(np.array([100, 200]), np.array([0, 300]), len(flows), seed=1)
    segs["reserved"] = [1, 4]
    dp, df, ds = engine.to_device(payload[:4096]), engine.to_device(flows), engine.to_device(segs)
    da, dl, dst = engine.alloc(64 * 64), engine.alloc(16), engine.alloc(32)
    do, dopt = engine.to_device(np.array([0, 8, 0, 0], np.uint32)), engine.to_device(opts)
    try:
        def call(opts_ptr=dopt.ptr, nopts=len(opts), **kw):
            a = dict(payload=dp.ptr, payload_bytes=4096, flows=df.ptr, nflows=len(flows), n=2, segs=ds.ptr,
                     frames=da.ptr, off64=do.ptr, slot0=0, stride64=0, len=dl.ptr, stats=dst.ptr)
            a.update(kw)
            b = rxg.DevTxBuildOpt(rxg.DevTxBuild(**a), opts_ptr, nopts, 0)
            return lib.rxg_tx_build_opt_dev(engine.ctx, C.byref(b), None)
        assert call() == 0
        engine.sync()
        for kw, why in [(dict(opts_ptr=dopt.ptr + 8), b"opts"), (dict(opts_ptr=dopt.ptr + 4), b"opts"),
                        (dict(opts_ptr=None), b"opts"), (dict(opts_ptr=None, nopts=1), b"opts"),
                        (dict(frames=da.ptr + 16), b"alignment"), (dict(segs=ds.ptr + 4), b"alignment"),
                        (dict(flows=df.ptr + 4), b"alignment"), (dict(off64=do.ptr + 2), b"alignment"),
                        (dict(len=dl.ptr + 1), b"alignment"), (dict(stats=dst.ptr + 4), b"alignment"),
                        (dict(payload=dp.ptr + 8), b"alignment"), (dict(off64=None, stride64=0), b"stride64"),
                        (dict(off64=None, slot0=0xFFFFFFFF, stride64=1), b"2^32"),
                        (dict(frames=None), b"NULL"), (dict(segs=None), b"NULL"), (dict(flows=None), b"NULL"),
                        (dict(len=None), b"NULL"), (dict(payload=None), b"NULL")]:
            assert call(**kw) == -EINVAL, kw
            err = lib.rxg_last_error()
            assert why in err and b"rxg_tx_build_opt_dev" in err, (kw, err)
        assert lib.rxg_tx_build_opt_dev(engine.ctx, None, None) == -EINVAL
        # n == 0 does nothing, whatever else is set; opts may be NULL with nopts 0; stats may be NULL
        assert call(n=0, frames=None, segs=None, opts_ptr=dopt.ptr + 1) == 0
        assert call(opts_ptr=None, nopts=0) == 0  # both segments name a block: skipped, not an error
        assert call(stats=None) == 0
        assert call(off64=None, slot0=0, stride64=8) == 0
        engine.sync()
        assert list(dl.download(np.uint16, 2)) == [54 + 0 + 100, 54 + 12 + 200]
    finally:
        for d in (dp, df, ds, da, dl, dst, do, dopt):
            d.free()
