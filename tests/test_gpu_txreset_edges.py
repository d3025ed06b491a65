"""GPU: rxg_tx_reset_dev on the deterministic sets of tests/txreset_cases.py -- the slice-count
scan past its first lanes, its waves and its rounds (up to 2 098 240 frames), stale slice counts
left by a larger call, a slice's reset count on every edge of the build pass's 16-reset rounds,
`cap` inside a slice, every offender length, the checksum corners -- against
txreset_cases.build_fast, which tests/test_txreset_cases_host.py pins to the reference model and
whose sets it holds to their claims.  The call is a pure function of its arguments, so the
records are written by the test in the documented layouts with random bits around the verdict;
the first test ties that to what a real burst writes.  Same discipline as test_gpu_txreset.py:
out, idx and count pre-filled with 0xA5, GUARD slots past cap, everything compared."""
import functools

import numpy as np
import pytest

import pktgen
import rxg
import txreset_cases as tc
from test_gpu_txreset import GUARD, Batch, Out, check

pytestmark = pytest.mark.gpu

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
ID0 = 0xFFF0       # the packet id wraps after 16 resets, and many times in the scan sizes
assert GUARD == tc.GUARD


class Dev:
    """A case's inputs on the device: the pool as the device is to see it, off64, len, records."""

    def __init__(self, eng, c, rec_kind=rxg.REC8):
        self.c, self.rec_kind = c, rec_kind
        self.bufs = [eng.to_device(np.ascontiguousarray(a)) for a in (c.dev_pool, c.off, c.lens, c.recs(rec_kind))]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.bufs:
            d.free()


def run(eng, d, cap, ip_id0, strided=None):
    pool, off, lens, recs = d.bufs
    o = Out(eng, cap)
    try:
        eng.tx_reset_dev(pool.ptr, lens.ptr, d.c.n, recs.ptr, d.rec_kind, o.out.ptr, o.idx.ptr, cap, o.count.ptr,
                         off64=None if strided else off.ptr, slot0=strided[0] if strided else 0,
                         stride64=strided[1] if strided else 0, ip_id0=ip_id0, src_mac=tc.MAC)
        eng.sync()
        return o.get()
    finally:
        o.free()


@pytest.fixture(scope="module")
def grids(engine):
    """The occupancy grid, and contexts whose launches are capped at 1 and 2 workgroups."""
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    yield [("occupancy grid", engine), ("max_blocks 1", e1), ("max_blocks 2", e2)]
    e1.close()
    e2.close()


rank_cases = functools.lru_cache(maxsize=None)(tc.rank_cases)


# --------------------------------------------- 1. the record helper against a real burst ---
@pytest.mark.parametrize("rec_kind", KINDS)
def test_verdict_of_reads_what_a_burst_writes(engine, rec_kind):
    rows, frames = pktgen.parity_set(seed=41, n=3000)
    tcb, live = pktgen.table_arrays(rows)
    b = Batch(engine, *pktgen.pack_arena(frames), rec_kind, tcb, live)
    try:
        got = tc.verdict_of(b.dr.download(np.uint8, b.n * rec_kind), rec_kind)
        assert set(b.verdicts.tolist()) == set(range(6))
        assert np.array_equal(got, b.verdicts)
    finally:
        b.close()


# ------------------------------------------------------------------------ 2. scan sizes ---
@pytest.mark.parametrize("nslices", tc.SCAN_NSLICES)
def test_scan_sizes_on_every_grid(grids, nslices):
    for n in tc.scan_n(nslices):
        c = tc.scan_case(nslices, n)
        want = c.want(c.count, ID0)
        with Dev(grids[0][1], c) as d:
            for gname, eng in grids:
                check(run(eng, d, c.count, ID0), want, c.count, f"{nslices} slices, n {n}, {gname}")


@pytest.mark.parametrize("rec_kind", [rxg.REC16, rxg.REC48])
@pytest.mark.parametrize("nslices", [tc.SCAN_ROUND - 1, tc.SCAN_ROUND + 1])
def test_scan_round_edge_in_the_wide_record_kinds(engine, nslices, rec_kind):
    c = tc.scan_case(nslices, tc.scan_n(nslices)[0])
    with Dev(engine, c, rec_kind) as d:
        check(run(engine, d, c.count, ID0), c.want(c.count, ID0), c.count, f"{nslices} slices, REC{rec_kind}")


# ---------------------------------------------------------------------- 3. stale counts ---
def test_a_smaller_call_ignores_the_counts_a_larger_one_left(engine):
    """The context's slice counts only grow.  A flood call of 16 385 slices (cap 0: nothing is
    written but the counts, which end as prefix sums up to 1 048 576) leaves its sums in the
    entries at and past a later, smaller call's nslices, inside that call's last 16-entry group."""
    with rxg.Engine(device=0) as eng:
        c = tc.flood_case(tc.STALE_FIRST)
        with Dev(eng, c) as d:
            check(run(eng, d, 0, ID0), c.want(0, ID0), 0, "flood")
        for nslices in tc.STALE_THEN:
            for n in tc.scan_n(nslices):
                c = tc.scan_case(nslices, n)
                with Dev(eng, c) as d:
                    check(run(eng, d, c.count, ID0), c.want(c.count, ID0), c.count, f"{nslices} slices after the flood")


# ------------------------------------------------------------- 4. rank, cap and length ---
@pytest.mark.parametrize("rec_kind", KINDS)
@pytest.mark.parametrize("name", ["low", "high", "spread", "holes", "single", "last1", "last63"])
def test_rank_cases(grids, name, rec_kind):
    c = rank_cases()[name]
    want = c.want(c.n, ID0)
    assert want[2] == c.count
    with Dev(grids[0][1], c, rec_kind) as d:
        for gname, eng in grids[:2]:
            check(run(eng, d, c.n, ID0), want, c.n, f"{name}, REC{rec_kind}, {gname}")


def test_rank_cases_strided(engine):
    for name, c in rank_cases().items():
        s = c.strided(3, 2)
        with Dev(engine, s) as d:
            check(run(engine, d, s.n, ID0, strided=(3, 2)), c.want(c.n, ID0), s.n, f"{name}, strided")


def test_cap_inside_a_slice(grids):
    c = tc.cap_case()
    with Dev(grids[0][1], c) as d:
        for cap in tc.caps():
            want = c.want(cap, ID0)
            assert want[2] == c.count and len(want[1]) == min(cap, c.count)
            for gname, eng in grids[:2]:
                check(run(eng, d, cap, ID0), want, cap, f"cap {cap}, {gname}")


def test_every_length_with_the_rest_of_the_line_poisoned(grids):
    c = tc.length_case()
    want = c.want(c.n, ID0)
    assert c.dev_pool is not c.pool and set(c.lens[want[1]].tolist()) == set(tc.LENGTHS)
    with Dev(grids[0][1], c) as d:
        for gname, eng in grids[:2]:
            check(run(eng, d, c.n, ID0), want, c.n, f"lengths, {gname}")


# --------------------------------------------------------------- 5. checksum corners ---
@pytest.mark.parametrize("rotation", range(len(tc.CORNER_KINDS)))
def test_checksum_corners(grids, rotation):
    c = tc.corner_case(rotation)
    want = c.want(c.n)
    with Dev(grids[0][1], c) as d:
        for gname, eng in grids[:2]:
            got = run(eng, d, c.n, c.ip_id0)
            check(got, want, c.n, f"rotation {rotation}, {gname}")
            lines = got[0].reshape(-1, 64)
            for kind, k in c.named.items():
                if kind in ("ip", "both"):
                    assert lines[k, 24:26].tolist() == [0, 0], (kind, k, gname)
                if kind in ("tcp", "both"):
                    assert lines[k, 50:52].tolist() == [0, 0], (kind, k, gname)
