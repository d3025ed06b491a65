"""GPU: rxg_flow_sums_dev on the edge sets of tests/flowsum_edge_cases.py -- two frames of one flow
meeting in the wave reduction, the register carry, the LDS merge, across workgroups, in per-lane
atomics, in atomics under a carried sum and after a commit on a flow change (each with unsigned
maxima at the sign bit, the first frame's state, all eight flag bits and an int32 datalen sum that
passes 2^32 there); every ending pattern of the LDS merge; slice runs around one, two and three
rounds of the waves; whole slices of left-out frames; every decoded field value per record kind;
frame lengths up to 0xFFFF in shuffled and strided pools; cap from 0 to 2^64 - 1; and the tile
scan at one round, beside it and at the largest table -- against the model tests/flowsum_ref.py,
never the kernel's own output or the host function (tests/test_flowsum_edge_cases_host.py pins
that one to the model on the same sets and holds the sets to their claims).  Contexts with
max_blocks 1, 2 and 3 and the default one: each run's bytes equal the model's, and the runs equal
each other.  Same discipline as test_gpu_flowsum.py: outputs pre-filled with 0xA5 and compared
whole, eight guard entries and the words around `count` included."""
import numpy as np
import pytest

import flowsum_edge_cases as ec
import rxg
from test_gpu_flowsum import FILL, GUARD, Batch

pytestmark = pytest.mark.gpu

assert GUARD == ec.GUARD


class EdgeBatch(Batch):
    """A Batch whose `out` always holds m + GUARD entries, whatever `cap` says."""

    def outs(self, cap=None):
        return (self.eng.to_device(np.full((self.m + GUARD) * 40, FILL, np.uint8)),
                self.eng.to_device(np.full(5 * 8, FILL, np.uint8)), self.m if cap is None else cap)

    def check(self, o, what=""):
        out, count, cap = o
        cw = count.download(np.uint64, 5)
        assert cw[0] == cw[4] == 0xA5A5A5A5A5A5A5A5, (what, "words around count were written")
        assert cw[1:4].tolist() == self.wcount.tolist(), (what, cw[1:4], self.wcount)
        got = out.download(np.uint8, (self.m + GUARD) * 40).view(rxg.FLOW_SUM_DTYPE)
        k = min(self.m, cap)
        if got[:k].tobytes() != self.want[:k].tobytes():
            bad = [i for i in range(k) if got[i] != self.want[i]]
            raise AssertionError(f"{what}: {len(bad)} of {k} summaries differ, first at {bad[0]}: got {got[bad[0]]} "
                                 f"want {self.want[bad[0]]}")
        assert (got[k:].view(np.uint8) == FILL).all(), (what, "entries at or past min(count, cap) were written")
        return got[:k].tobytes() + cw[1:4].tobytes()

    def repool(self, pool, off, lens, geom):
        """The same frames in another pool."""
        self.da, self.do, self.dl, self.geom = self.up(pool), self.up(off), self.up(lens), geom


def batch_of(eng, c, kind):
    return EdgeBatch(eng, kind, c.ntcb, rec48=c.rec48, frames=c.frames(kind), flags=c.flags, no_frames=kind == rxg.REC48)


@pytest.fixture(scope="module")
def ctx(engine):
    """max_blocks -> context; 0: the default grid."""
    made = {mb: rxg.Engine(device=0, max_blocks=mb) for mb in ec.BLOCKS}
    yield {0: engine, **made}
    for e in made.values():
        e.close()


def run_case(ctx, c, blocks=None, **kw):
    """The case in each of its kinds on the default context and every max_blocks it names: each
    equals the model, and they equal each other."""
    for kind in c.kinds:
        b = batch_of(ctx[0], c, kind)
        try:
            got = [b.run(ctx[mb], what=f"{c.name}, records of {kind}, max_blocks {mb or 'default'}", **kw)
                   for mb in [0] + list(blocks or c.blocks)]
            assert all(g == got[0] for g in got)
        finally:
            b.close()


# ------------------------------------------------ 1. where two frames of a flow meet ---
@pytest.mark.parametrize("mb", ec.BLOCKS)
@pytest.mark.parametrize("place", ec.PLACES)
def test_meet(ctx, place, mb):
    for c in ec.meet_cases(place, mb):
        run_case(ctx, c)


# ------------------------------------------------------ 2. the workgroup's LDS merge ---
@pytest.mark.parametrize("pattern", ec.LDS_PATTERNS)
def test_lds_merge_endings(ctx, pattern):
    for kind in ec.KINDS:
        run_case(ctx, ec.lds_case(pattern, kind), blocks=ec.BLOCKS)


# --------------------------------------------------------------- 3. a wave's slice run ---
@pytest.mark.parametrize("mb", ec.BLOCKS)
def test_slice_runs(ctx, mb):
    for c in ec.run_cases(mb):
        run_case(ctx, c)


# ------------------------------------------------------- 4. the two left-out counters ---
@pytest.mark.parametrize("c", ec.left_cases(), ids=repr)
def test_left_out_counters(ctx, c):
    run_case(ctx, c)


# --------------------------------------------------------------- 5. the record decode ---
@pytest.mark.parametrize("kind", ec.KINDS)
def test_decode(ctx, kind):
    run_case(ctx, ec.decode_case(kind))


# ------------------------------------------------- 6. seq and ack read from the frame ---
@pytest.mark.parametrize("form", range(6), ids=[name for name, _, _ in ec.frame_forms()])
def test_frame_lengths_and_pools(ctx, form):
    name, c, build = ec.frame_forms()[form]
    for kind in c.kinds:
        b = batch_of(ctx[0], c, kind)
        try:
            pool, off, lens, geom = build(c.frames(kind))
            b.repool(pool, off, lens, geom)
            got = [b.run(ctx[mb], what=f"{name}, records of {kind}, max_blocks {mb or 'default'}", use_stride=st)
                   for mb in (0, 1, 2) for st in ([False, True] if geom else [False])]
            assert all(g == got[0] for g in got)
        finally:
            b.close()


# --------------------------------------------------------------- 7. the output limit ---
@pytest.mark.parametrize("kind", ec.KINDS)
def test_cap(ctx, kind):
    c = ec.cap_case(kind)
    b = batch_of(ctx[0], c, kind)
    try:
        assert b.m == 150
        for mb, eng in ctx.items():
            full = b.run(eng, what=f"max_blocks {mb or 'default'}")
            for cap in ec.caps(b.m):
                cut = b.run(eng, cap=cap, what=f"cap {cap}, max_blocks {mb or 'default'}")
                assert cut[:-24] == full[:min(cap, b.m) * 40]
                # the cut call left accumulator and bitmap all zero, past cap too
                assert b.run(eng, what=f"after cap {cap}, max_blocks {mb or 'default'}") == full
    finally:
        b.close()


# ------------------------------------------------------------------- 8. the tile scan ---
@pytest.mark.parametrize("ntcb", ec.SCAN_NTCB)
def test_scan_rounds(ctx, ntcb):
    c = ec.scan_case(ntcb)
    run_case(ctx, c, blocks=[1] if ntcb == rxg.FS_MAX_NTCB else ec.BLOCKS)
