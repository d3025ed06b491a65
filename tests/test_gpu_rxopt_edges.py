"""GPU: rxg_rx_opts_dev on the edge sets of tests/rxopt_edge_cases.py -- every len 0..130, 1 514
and 65 535 at every data_off nibble, the chunk-5 test on every edge lane, every verdict on every
lane in all three record layouts, every round count of the walk 1..40 in one slice and a 40-round
lane beside lanes that are done at once or never walk, the three bad-length tests at every
(O, p, l), SACK at every offset, the aligned-timestamp compare and its 32 neighbours, and batches
that give a wave a second and third slice -- against the model tests/rxopt_ref.py, never the
kernel's own output or the host parser (tests/test_rxopt_edge_cases_host.py pins that one to the
model on the same frames and holds the sets to their claims).  The call is a pure function of
frames and records, so the records are written by the test in the documented layouts with random
bits around the verdict; the first test ties that to what a real burst writes.  Same discipline
as test_gpu_rxopt.py: outputs pre-filled with 0xA5 and compared whole, eight guard records past n
included; what follows a frame's last byte in the pool parses as valid options."""
import numpy as np
import pytest

import pktgen
import rxg
import rxopt_edge_cases as ec
import rxopt_ref as ref
import txreset_cases as tc
from test_gpu_rxopt import FILL, GUARD, Batch

pytestmark = pytest.mark.gpu

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
assert GUARD == ec.GUARD


class Dev:
    """A call's inputs on the device: pool, off64, len and the records the test wrote."""

    def __init__(self, eng, pool, off, lens, recs, rec_kind, geom=None):
        self.n, self.rec_kind, self.geom = len(lens), rec_kind, geom
        self.bufs = [eng.to_device(np.ascontiguousarray(a)) for a in (pool, off, lens, recs)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.bufs:
            d.free()

    def run(self, eng, use_stride=False) -> np.ndarray:
        """The whole output buffer, guards included, after one call."""
        pool, off, lens, recs = self.bufs
        out = eng.to_device(np.full((self.n + GUARD) * 16, FILL, np.uint8))
        try:
            eng.rx_opts_dev(pool.ptr, lens.ptr, self.n, recs.ptr, self.rec_kind, out.ptr,
                            off64=None if use_stride else off.ptr, slot0=self.geom[0] if use_stride else 0,
                            stride64=self.geom[1] if use_stride else 0)
            eng.sync()
            return out.download(np.uint8, (self.n + GUARD) * 16)
        finally:
            out.free()


def check(raw, want, what, describe):
    n = len(want)
    assert (raw[n * 16:] == FILL).all(), (what, "records past n were written")
    got = raw[:n * 16].view(rxg.RX_OPT_DTYPE)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {n} records differ, first at packet {i} (lane {i % 64}, "
                             f"{describe(i)}): got {got[i]} want {want[i]}")
    return raw


def run_case(eng, c, rec_kind=rxg.REC8, strided=False, seed=0, engines=None):
    """One set through the offset list or the fixed stride, on `eng` or on each of `engines`."""
    def describe(i):
        f = c.frames[i]
        return f"len {len(f)}, verdict {int(c.verdicts[i])}, meta {c.meta[i]}, bytes 46.. {f[46:94].hex()}"

    if strided:
        pool, off, lens, geom = c.strided()
    else:
        (pool, off, lens), geom = c.packed(), None
    with Dev(eng, pool, off, lens, c.recs(rec_kind, seed), rec_kind, geom) as d:
        return [check(d.run(e, use_stride=strided), c.want, f"{c.name}, REC{rec_kind}, {'stride' if strided else 'list'}, {name}",
                      describe) for name, e in (engines or [("", eng)])]


@pytest.fixture(scope="module")
def grids(engine):
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    e1.close()
    e2.close()


# --------------------------------------------- 1. the written records against a real burst ---
@pytest.mark.parametrize("rec_kind", KINDS)
def test_verdict_of_reads_what_a_burst_writes(engine, rec_kind):
    """300 frames a real burst classifies: the verdicts read back from its records with the reader
    of the layouts the sets write equal the oracle's; and the option pass on those records gives
    the model's answer."""
    rows, frames = pktgen.parity_set(31, 300)
    b = Batch(engine, frames, rec_kind, table=pktgen.table_arrays(rows))
    try:
        got = tc.verdict_of(b.dr.download(np.uint8, b.n * rec_kind), rec_kind)
        assert np.array_equal(got, b.verdicts)
        assert set(ref.CANDIDATE_VERDICTS) <= set(got.tolist()) and not set(got.tolist()) <= set(ref.CANDIDATE_VERDICTS)
        synthetic = tc.verdict_of(tc.make_recs(b.verdicts, rec_kind, 3), rec_kind)
        assert np.array_equal(synthetic, got)
        b.run(what=f"a real burst's records of {rec_kind}")
    finally:
        b.close()


# ------------------------------------------------------------ 2. lengths, rounds, verdicts ---
@pytest.mark.parametrize("strided", [False, True], ids=["list", "stride"])
@pytest.mark.parametrize("rec_kind", KINDS)
def test_len_grid(engine, rec_kind, strided):
    run_case(engine, ec.get("len_grid"), rec_kind, strided)
    run_case(engine, ec.get("len_grid_long"), rec_kind, strided)


@pytest.mark.parametrize("strided", [False, True], ids=["list", "stride"])
@pytest.mark.parametrize("rec_kind", KINDS)
def test_rounds(engine, rec_kind, strided):
    run_case(engine, ec.get("rounds"), rec_kind, strided)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("rec_kind", KINDS)
def test_verdicts(engine, rec_kind, seed):
    c = ec.get("verdicts")
    assert not c.want[~np.isin(c.verdicts, ec.CAND)].view(np.uint8).any()
    run_case(engine, c, rec_kind, seed=seed)
    run_case(engine, c, rec_kind, strided=True, seed=seed)


def test_len_grid_and_rounds_on_capped_grids(grids):
    for name in ("len_grid", "rounds"):
        raws = run_case(grids[0][1], ec.get(name), engines=grids)
        assert raws[0].tobytes() == raws[1].tobytes() == raws[2].tobytes()


# ------------------------------------------ 3. bad lengths, SACK offsets, the aligned compare ---
@pytest.mark.parametrize("size", ec.OPT_SIZES)
def test_length_tests(engine, size):
    run_case(engine, ec.length_tests(size))


def test_sack_grid(engine):
    run_case(engine, ec.get("sack_grid"))


@pytest.mark.parametrize("rec_kind", KINDS)
def test_aligned_edges(engine, rec_kind):
    run_case(engine, ec.get("aligned_edges"), rec_kind)
    run_case(engine, ec.get("aligned_edges"), rec_kind, strided=True)


# ----------------------------------------------------------------------- 4. the grid stride ---
def describe_grid(g):
    return lambda i: f"slot {int(g.slot[i])}, len {int(g.lens[i])}, verdict {int(g.verdicts[i])}, bytes 46.. {g.frame(i)[46:94].hex()}"


@pytest.mark.parametrize("n", ec.GRID_SIZES)
def test_grid_sizes_on_capped_grids(grids, n):
    g = ec.GridCase(n)
    with Dev(grids[0][1], g.pool(), g.off, g.lens, g.recs(rxg.REC8), rxg.REC8) as d:
        raws = [check(d.run(eng), g.want, f"n {n}, {name}", describe_grid(g)).tobytes() for name, eng in grids]
    assert raws[0] == raws[1] == raws[2]


def test_grid_strided(grids):
    g = ec.GridCase(769)
    pool, geom = g.strided()
    with Dev(grids[0][1], pool, g.off, g.lens, g.recs(rxg.REC16), rxg.REC16, geom) as d:
        raws = [check(d.run(eng, use_stride=True), g.want, f"n 769 strided, {name}", describe_grid(g)).tobytes()
                for name, eng in grids]
    assert raws[0] == raws[1] == raws[2]


def test_grid_large_on_every_grid(grids):
    """2^20 + 81 frames: 16 386 slices, two or three per wave of the occupancy grid."""
    import torch
    n = ec.GRID_LARGE
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n > cus * ec.RESIDENT_WORKGROUPS * 256, cus      # every resident wave takes a second slice
    g = ec.GridCase(n)
    with Dev(grids[0][1], g.pool(), g.off, g.lens, g.recs(rxg.REC8), rxg.REC8) as d:
        raws = [check(d.run(eng), g.want, f"n {n}, {name}", describe_grid(g)).tobytes() for name, eng in grids]
    assert raws[0] == raws[1] == raws[2]


@pytest.mark.parametrize("rec_kind", [rxg.REC16, rxg.REC48])
def test_grid_large_in_the_wide_record_kinds(engine, rec_kind):
    g = ec.GridCase(ec.GRID_LARGE)
    with Dev(engine, g.pool(), g.off, g.lens, g.recs(rec_kind), rec_kind) as d:
        check(d.run(engine), g.want, f"n {g.n}, REC{rec_kind}", describe_grid(g))
