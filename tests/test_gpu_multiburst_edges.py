"""GPU: the multi-burst launch (rxg_rx_bursts_dev, rxg_rx_bursts_strided_dev) on the edge sets of
tests/multiburst_cases.py -- every ordered pair of burst sizes 1, 63, 64, 65 and 129 in one launch,
empty bursts in every position with valid and with NULL pointers, 1 to 97 bursts per call (32 in
one launch, a launch of one burst behind full ones, launch chunks that are entirely empty), record
rings that flush slots of several bursts before a wave ends, all-small runs that end on every kind
of burst edge one and two slices ahead, and bursts whose buffers lie in reverse order or in two
allocations -- on grids of one and two workgroups and the occupancy grid, in the record kinds the
set names, through the offset list and the fixed stride.  Every comparison covers the whole record
buffer (pre-filled with 0xA5, eight guard records behind every burst, the REC8 buffer 8 but not 16
bytes aligned) and the counters, against oracle.rx_batch over the bursts' concatenation.
tests/test_multiburst_cases_host.py holds the sets and the model of the dealing to their claims."""
import numpy as np
import pytest

import multiburst_cases as mc
import rxg

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("strided", [False, True], ids=["list", "stride"])
KINDS2 = pytest.mark.parametrize("kind", [rxg.REC8, rxg.REC16])
KINDS3 = pytest.mark.parametrize("kind", [rxg.REC8, rxg.REC16, rxg.REC48])
FAR_BYTES = 1 << 32


@pytest.fixture(scope="module")
def grids(engine):
    e1, e2 = rxg.Engine(device=0, max_blocks=1), rxg.Engine(device=0, max_blocks=2)
    gs = [("max_blocks 1", e1), ("max_blocks 2", e2), ("occupancy grid", engine)]
    for _, e in gs:
        e.tcb_load(mc.TCB, mc.LIVE)
        e.tcb_sync()
        e.arp_disable()
    yield gs
    e1.close()
    e2.close()


class Dev:
    """A case's pool, descriptors and record buffers on the device."""

    def __init__(self, eng, c, kind, strided):
        self.c, self.kind, self.strided = c, kind, strided
        off_all, len_all, self.start = c.desc
        self.pool = eng.to_device(c.strided if strided else c.packed[0])
        self.off, self.len = eng.to_device(off_all), eng.to_device(len_all)
        self.where, self.size = c.rec_layout(kind)
        if c.split:      # one allocation: the second record buffer 4 GiB above the first
            self.own = [eng.alloc(FAR_BYTES + self.size[1])]
            self.rec = [self.own[0].ptr, self.own[0].ptr + FAR_BYTES]
            assert self.size[0] < FAR_BYTES
        else:
            self.own = [eng.alloc(self.size[0])]
            self.rec = [self.own[0].ptr]
        assert all(r % 256 == 0 for r in self.rec)      # what the layout's alignment claims build on

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in [self.pool, self.off, self.len] + self.own:
            d.free()

    def bursts(self):
        c, out = self.c, []
        for j in range(c.k):
            b, o = self.where[j]
            if c.ns[j] == 0 and c.null_empties:
                ptrs = (None, None, None)
            else:
                ptrs = (self.off.ptr + 4 * self.start[j], self.len.ptr + 2 * self.start[j], self.rec[b] + o)
            out.append((c.slot0(j) if self.strided else ptrs[0], ptrs[1], c.ns[j], ptrs[2]))
        return out

    def run(self, eng):
        """One call: the record buffers whole, and the counters."""
        for r, s in zip(self.rec, self.size):
            fill = np.full(s, mc.FILL, np.uint8)
            eng.h2d(r, fill.ctypes.data, s)
            eng.sync()
        eng.counters_reset()
        eng.sync()
        if self.strided:
            eng.rx_bursts_strided_dev(self.pool.ptr, self.c.stride64, self.bursts(), self.kind)
        else:
            eng.rx_bursts_dev(self.pool.ptr, self.bursts(), self.kind)      # (raises unless the call returns 0)
        eng.sync()
        got = [np.empty(s, np.uint8) for s in self.size]
        for r, g in zip(self.rec, got):
            eng.d2h(g.ctypes.data, r, g.nbytes)
        eng.sync()
        return got, eng.counters()


def check(c, kind, what, got, cnt):
    imgs, ecnt = c.expect(kind)
    for b, (g, e) in enumerate(zip(got, imgs)):
        if g.tobytes() != e.tobytes():
            bad = np.nonzero(g != e)[0]
            at = int(bad[0])
            r = at // kind * kind if kind != rxg.REC8 else (at - 8) // 8 * 8 + 8
            raise AssertionError(f"{what}: {len(bad)} bytes of record buffer {b} differ, first at byte {at}: "
                                 f"{c.describe(kind, b, at)}: got {g[r:r + kind].tobytes().hex()} "
                                 f"want {e[r:r + kind].tobytes().hex()}")
    assert cnt.tolist() == ecnt.tolist(), (what, dict(zip(rxg.COUNTERS, zip(cnt.tolist(), ecnt.tolist()))))


def run_case(grids, name, kind, strided):
    c = mc.get(name)
    with Dev(grids[0][1], c, kind, strided) as d:
        for gname, eng in grids:
            got, cnt = d.run(eng)
            check(c, kind, f"{name}, REC{kind}, {'stride' if strided else 'list'}, {gname}", got, cnt)
    return c


@FORMS
@KINDS3
def test_pairs(grids, kind, strided):
    """Every ordered pair of the burst sizes next to each other in one launch of 26 bursts, all
    small and with a 65-byte frame closing every burst (its last slice on the class path)."""
    for name in mc.NAMES["pairs"]:
        run_case(grids, name, kind, strided)


@FORMS
@KINDS2
def test_empties(grids, kind, strided):
    """Empty bursts first, last, two in a row, all but one (the one left is not bursts[0] and runs
    the single-burst kernel) and all (nothing launched: the buffer keeps its fill and the counters
    stay zero), with valid and with NULL pointers."""
    for name in mc.NAMES["empties"]:
        c = run_case(grids, name, kind, strided)
        if "/all/" in name:
            assert not c.launches and all((img == mc.FILL).all() for img in c.expect(kind)[0])
            assert not c.expect(kind)[1].any()


@FORMS
@KINDS3
@pytest.mark.parametrize("n", mc.COUNT_NS)
def test_counts(grids, kind, strided, n):
    """1 to 97 bursts of one frame and of 65: 32 in a launch reads lane 31 of the burst table, 33
    and 65 leave one burst to the last launch, 97 takes four."""
    for k in mc.COUNT_KS:
        run_case(grids, f"counts/{k}/{n}", kind, strided)


@FORMS
@KINDS3
def test_counts_with_empty_chunks(grids, kind, strided):
    """64 bursts whose first or second 32 are all empty (that launch is not made), and 40 with
    the empty ones on both sides of the cut between the launches."""
    for h in mc.COUNT_HOLES:
        run_case(grids, f"counts/{h}", kind, strided)


@FORMS
@KINDS3
@pytest.mark.parametrize("name", mc.NAMES["ring"])
def test_ring(grids, kind, strided, name):
    """Launches in which a wave's ring flushes slots of several bursts, a burst's partial last slice
    among them, before the wave's end (which kernels and kinds: the host file, from the model)."""
    run_case(grids, name, kind, strided)


@FORMS
@KINDS2
@pytest.mark.parametrize("name", mc.NAMES["runs"])
def test_runs(grids, kind, strided, name):
    """All-small runs whose look-ahead meets a full slice of the next burst, a partial one, a
    65-byte frame on lane 0 or 63, a one-frame burst and the launch's end, one slice ahead and, in
    the launch of 67 slices on one workgroup, two slices ahead with and without a pending slice."""
    run_case(grids, name, kind, strided)


@FORMS
@KINDS2
def test_order_reversed(grids, kind, strided):
    """The bursts of `pairs` with their three ranges in reverse order in memory."""
    run_case(grids, "order/reversed", kind, strided)


@KINDS2
def test_order_two_allocations(grids, kind, capsys):
    """The same with every second burst's records in a second buffer 4 GiB above the first, both
    in one allocation, so that the `out` pointers of one launch differ above bit 31 (both halves of
    BurstCursor::rl_ptr carry information).  Nothing is asserted about the addresses; the MI355X
    run of this test printed the high dwords 0x72f8 and 0x72f9."""
    c = mc.get("order/split")
    for strided in (False, True):
        with Dev(grids[0][1], c, kind, strided) as d:
            with capsys.disabled():
                print(f"\norder/split REC{kind}: record buffers at {d.rec[0]:#x} and {d.rec[1]:#x}, "
                      f"high dwords {d.rec[0] >> 32:#x} and {d.rec[1] >> 32:#x}")
            for gname, eng in grids:
                got, cnt = d.run(eng)
                check(c, kind, f"order/split, REC{kind}, {'stride' if strided else 'list'}, {gname}", got, cnt)
