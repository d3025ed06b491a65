"""GPU: rxg_tx_build_opt_dev on the deterministic sets of tests/txbuild_opt_cases.py -- every
block length 0, 4, .. 40 at the edges of the option instantiation's own code: both byte masks
in one chunk, the block's chunks in frame chunks 3, 4 and 5, the source clamp at the buffer's
two ends, streamed frames without data, the one-line path with a block, size classes by O + L,
the block index through the group broadcast.  What each set holds is asserted on the CPU in
tests/test_txbuild_opt_cases_host.py.  As in test_gpu_txbuild_opt.py every expectation is the
model's (txbuild_opt_ref.build, the oracle's checksums), every pool is pre-filled with 0xA5
and compared whole, byte for byte, with len and stats."""
import numpy as np
import pytest

import rxg
import rxopt_ref
import txbuild_opt_cases as cases
import txbuild_opt_ref as oref
from test_gpu_txbuild_opt import check, explain, run_opt

pytestmark = pytest.mark.gpu

ALL = oref.ALL_OPT_LENS
FILL = cases.FILL
GUARD = 8
HDR = 54


def check_case(eng, c, what="", model=None, **kw):
    return check(eng, *c.args, what, model or c.model(), **c.kw, **kw)


@pytest.fixture(scope="module")
def grids(engine):
    """Contexts whose launches are capped at 1 and 2 workgroups, and the occupancy grid."""
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    e1.close()
    e2.close()


def on_every_grid(grids, c):
    """The same pool from grids of 1 and 2 workgroups (a wave takes several slices) and the
    occupancy grid, added to stats that are not zero."""
    model = c.model()
    pools = [check_case(eng, c, name, model, stats0=(5, 7)) for name, eng in grids]
    assert np.array_equal(pools[0], pools[1]) and np.array_equal(pools[0], pools[2])
    return pools[2]


# ------------------------------------------------------------------------- masks ---
@pytest.mark.parametrize("O", ALL)
def test_masks_by_offset_list_and_by_stride(engine, O):
    """Every tail residue at every source shift, every data_len 0..48 at every alignment:
    through off64 in a random order, and through a fixed stride of equal slots."""
    c = cases.masks(O)
    check_case(engine, c, f"O {O}, off64")
    n, slot0, stride64 = len(c.segs), 3, c.labels["stride64"]
    off = (slot0 + np.arange(n) * stride64).astype(np.uint32)
    nslots = slot0 + n * stride64 + 1
    want, wlen, wstats = oref.build(c.payload, c.flows, c.segs, c.opts, off, nslots, fill=FILL)
    got, glen, gstats = run_opt(engine, c.payload, c.flows, c.segs, c.opts, nslots, slot0=slot0, stride64=stride64)
    assert np.array_equal(glen, wlen) and list(gstats) == list(wstats) == [n, 0]
    assert np.array_equal(got, want), f"O {O}, stride " + explain(got, want, off, wlen, c.segs)


# ------------------------------------------------------------------- class_edges ---
@pytest.fixture(scope="module")
def edges():
    return cases.class_edges()


def test_class_edges_on_every_grid(grids, edges):
    assert set(edges.labels["O"].tolist()) == set(ALL) and len(edges.segs) > 64 * 4 * 2
    on_every_grid(grids, edges)


def test_class_edges_through_the_receive_path_and_the_option_parse(engine, edges):
    """The built frames classify as DISPATCH with both checksums 0 and data_off (5 + O / 4) << 4
    on the shipped receive path, and rxg_rx_opts_dev reads the blocks' options back."""
    c = edges
    n = len(c.segs)
    ol = c.labels["O"]
    pool, flen, stats = run_opt(engine, *c.args[:4], c.nslots, off64=c.off64)
    assert list(stats) == [n, 0] and np.array_equal(flen, oref.frame_lens(c.segs["data_len"], ol))
    frames = [pool[int(o) * 64:int(o) * 64 + int(k)].tobytes() for o, k in zip(c.off64, flen)]
    with rxg.Engine(device=0) as peer:
        peer.tcb_load(cases.peer_tcbs(c.flows), np.ones(len(c.flows), np.uint8))
        da, do, dl = peer.to_device(pool), peer.to_device(c.off64), peer.to_device(flen)
        dr = peer.to_device(np.full(n * rxg.REC48, FILL, np.uint8))
        out = peer.to_device(np.full((n + GUARD) * 16, FILL, np.uint8))
        try:
            peer.rx_burst_dev(da.ptr, do.ptr, dl.ptr, n, dr.ptr, rxg.REC48)
            peer.rx_opts_dev(da.ptr, dl.ptr, n, dr.ptr, rxg.REC48, out.ptr, off64=do.ptr)
            peer.sync()
            recs = dr.download(rxg.rec_dtype(rxg.REC48), n)
            raw = out.download(np.uint8, (n + GUARD) * 16)
        finally:
            for d in (da, do, dl, dr, out):
                d.free()
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all()
    assert (recs["c"]["flags"] & (rxg.F_IP_OK | rxg.F_TCP_OK) == rxg.F_IP_OK | rxg.F_TCP_OK).all()
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert np.array_equal(recs["c"]["tcb_idx"], c.segs["flow"].astype(np.int32))
    assert np.array_equal(recs["c"]["datalen"], c.segs["data_len"].astype(np.int32))
    assert np.array_equal(recs["data_off"], ((5 + ol // 4) << 4).astype(np.uint8))
    assert np.array_equal(recs["seq"], c.segs["seq"]) and np.array_equal(recs["ack"], c.segs["ack"])
    assert (raw[n * 16:] == FILL).all()
    got = raw[:n * 16].view(rxg.RX_OPT_DTYPE)
    assert np.array_equal(got["opt_len"], ol.astype(np.uint8))
    want = rxopt_ref.records(frames, recs["c"]["verdict"])
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"{len(bad)} records differ, first {int(bad[0])}: got {got[bad[0]]} want {want[bad[0]]}"
    for O in ALL:  # what went in: the fields of the block's real options
        w = rxopt_ref.parse(bytes(46) + bytes([(5 + O // 4) << 4]) + bytes(7) + cases.REAL_OPTIONS[O])
        mine = got[ol == O]
        for f in ("tsval", "tsecr", "mss", "wscale", "nsack", "sack_off", "opt_len", "flags"):
            assert (mine[f] == w[f]).all(), (O, f)
    again = engine.tx_arena(pool, c.off64, flen)
    assert np.array_equal(again, pool)


# ------------------------------------------------------------------------ slices ---
@pytest.mark.parametrize("cls", cases.CLASSES)
def test_slices_of_one_class(engine, cls):
    """Two full slices of one class, O mixed (m == ~0: no lane compaction), and one of 17."""
    check_case(engine, cases.slices(cls), f"class {cls}")


def test_slices_all_on_every_grid(grids):
    """Full slices of every class, the slice of all six classes whose counts end inside a
    round, 64 lanes naming 64 blocks and one block, skipped descriptors on lanes 0, 31, 32 and
    63, a last slice of 17."""
    c = cases.slices_all()
    got = on_every_grid(grids, c)
    for i in np.nonzero(c.labels["skipped"])[0]:  # said on its own: a skipped descriptor's slot is untouched
        a = int(c.off64[i]) * 64
        assert (got[a:a + 64] == FILL).all(), i


# ------------------------------------------------------------------ surroundings ---
@pytest.mark.parametrize("inside,outside", cases.FORMS)
@pytest.mark.parametrize("O", ALL)
def test_segment_and_block_bytes_against_their_surroundings(engine, inside, outside, O):
    """0xFF inside drives each 16-bit add to its largest value; 0x00 inside shows any byte
    taken from outside [src_off, src_off + L), from a block at or past `len` or from its
    reserved fields in the frame's padding and in its checksum."""
    check_case(engine, cases.surroundings(inside, outside, O), f"O {O}")


def test_single_option_bytes(engine):
    """Block byte j alone 0xFF: frame byte 54 + j and the checksum, nothing else."""
    c = cases.single_bytes()
    got = check_case(engine, c)
    zero = got[int(c.off64[0]) * 64:int(c.off64[0]) * 64 + 128]
    for j in range(40):
        a = int(c.off64[1 + j]) * 64
        diff = set(np.nonzero(got[a:a + 128] != zero)[0].tolist())
        assert HDR + j in diff and diff <= {50, 51, HDR + j}, j


# ------------------------------------------------------------------ payload ends ---
@pytest.mark.parametrize("O", ALL)
def test_segments_at_the_payload_start(engine, O):
    """src_off 0..15: the first source chunk lies up to 48 bytes before the payload."""
    check_case(engine, cases.payload_starts(O), f"O {O}")


@pytest.mark.parametrize("pbytes", cases.END_BYTES)
def test_segments_ending_at_payload_bytes(engine, pbytes):
    """Every edge length behind every block ending exactly at payload_bytes (data_len 0:
    src_off == payload_bytes), 0xEE from there to the buffer's end: none may show in a frame."""
    c = cases.payload_ends(pbytes)
    got = check_case(engine, c, f"payload_bytes {pbytes}")
    ol, dl = c.labels["O"], c.segs["data_len"]
    for i in range(len(dl)):  # said on its own: the payload bytes are the source's last L
        a = int(c.off64[i]) * 64 + HDR + int(ol[i])
        assert np.array_equal(got[a:a + int(dl[i])], c.payload[pbytes - int(dl[i]):pbytes]), i


@pytest.mark.parametrize("O", ALL[1:])
def test_longest_segments(engine, O):
    """RXG_TX_MAX_DATA - O, the source shift zero and not."""
    c = cases.longest(O)
    got = check_case(engine, c, f"O {O}")
    assert int(c.segs["data_len"][0]) == rxg.TX_MAX_DATA - O and c.nslots * 64 > 2 * 65535
    assert (got[(c.nslots - 1) * 64:] == FILL).all()


# --------------------------------------------------------------------- checksums ---
def test_checksum_corners(engine):
    """Stored TCP checksums of 0x0000 by an option word of chunk 3, 4 and 5 in every class,
    an IP header checksum of 0x0000 under a block, the largest sum, a sum that carries after
    one fold."""
    c = cases.checksums()
    got = check_case(engine, c)
    for i in range(6):
        a = int(c.off64[i]) * 64
        assert not got[a + 50:a + 52].any(), i
    a = int(c.off64[cases.I_IP]) * 64
    assert not got[a + 24:a + 26].any()
