"""GPU parity of the receive checksum span on the deterministic sets of rxspan_cases.py: the end
of the TCP span at every chunk and lane boundary of every size class (fields_small, the eight
streaming classes of frame_round_compute with their wave-uniform slow-span branch and per-frame
select, frame_fields<64, 2, JUMBO>), through every entry point that runs those routines --
launched bursts on the full and on a capped grid, tx checksum generate, the fused payload
hand-off copied and by reference, the resident server -- plus one-bit flips at every byte and
the largest sums.  Every comparison is bit-exact with the oracle; no tolerance anywhere.
"""
import functools

import numpy as np
import pytest

import oracle
import pktgen
import rxg
import rxspan_cases as cases

pytestmark = pytest.mark.gpu

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
FILL = 0x5C  # the payload arena's bytes before a copying hand-off


@pytest.fixture(scope="module", params=[1, 3])
def capped_engine(request):
    """A context whose rx grid is 1 or 3 workgroups (rxg_config.max_blocks): 4 or 12 waves walk
    the whole set, so a wave runs many rounds of one class back to back."""
    eng = rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20, max_blocks=request.param)
    yield eng
    eng.close()


class Case:
    """A set packed once, with the oracle's answer (left unchanged by the tests sharing it)."""

    def __init__(self, rows, frames):
        self.frames = frames
        self.arena, self.off, self.lens = pktgen.pack_arena(frames)
        self.tcb, self.live = pktgen.table_arrays(rows)
        self.exp, self.ecnt = oracle.rx_batch(self.arena, self.off, self.lens, self.tcb, self.live)
        for a in (self.arena, self.off, self.lens, self.exp, self.ecnt):
            a.setflags(write=False)

    def want(self, rec_kind, lo=0, hi=None):
        e = self.exp[lo:hi]
        return e if rec_kind == rxg.REC48 else e["c"] if rec_kind == rxg.REC16 else rxg.rec8_pack(e["c"])


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "grid":
        return Case(*cases.span_grid())
    if name == "interleaved":
        return Case(*cases.span_grid_interleaved())
    if name in ("all_small", "small_mixed"):
        rows, all_small, mixed = cases.small_layouts()
        return Case(rows, all_small if name == "all_small" else mixed)
    if name in ("flip0", "flip40"):
        rows, frames, base_of = cases.flip_set(int(name[4:]))
        c = Case(rows, frames)
        c.base_of = base_of
        return c
    assert name == "extreme"
    rows, frames, kinds = cases.extreme_set()
    c = Case(rows, frames)
    c.kinds = kinds
    return c


def assert_records(got, want, frames, what, first=0):
    """Bit-exact, and the first differing frame named by its cell."""
    if got.tobytes() == want.tobytes():
        return
    n = len(frames)
    gb = np.ascontiguousarray(got).view(np.uint8).reshape(n, -1)
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(n, -1)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    i = int(bad[0])
    raise AssertionError(f"{what}: records differ at {len(bad)} of {n} frames, first frame {first + i} "
                         f"({cases.describe(frames[i])}, slice {(first + i) // 64}, lane {(first + i) % 64}): "
                         f"got {got[i]} exp {want[i]}")


def run_rx(eng, c, rec_kind, what):
    eng.tcb_load(c.tcb, c.live)
    eng.counters_reset()
    got = eng.rx_arena(c.arena, c.off, c.lens, rec_kind)
    cnt = eng.counters()
    assert_records(got, c.want(rec_kind), c.frames, what)
    assert np.array_equal(cnt, c.ecnt), (what, cnt, c.ecnt)
    return got


# ------------------------------------------------------------------ the grid, launched ---

@pytest.mark.parametrize("rec_kind", KINDS)
@pytest.mark.parametrize("order", ["grid", "interleaved"])
def test_grid_full_grid(engine, order, rec_kind):
    """Both orderings (rounds uniformly slow-span or fast; rounds whose frames disagree) on the
    occupancy grid, every record kind (REC8: rxg.rec8_pack of the oracle's records)."""
    run_rx(engine, case(order), rec_kind, f"{order} REC{rec_kind}")


@pytest.mark.parametrize("order", ["grid", "interleaved"])
def test_grid_capped_grid(capped_engine, order):
    """One or three workgroups walk all 14 964 frames: many rounds of a class back to back."""
    run_rx(capped_engine, case(order), rxg.REC16, f"{order} capped REC16")


@pytest.mark.parametrize("rec_kind", KINDS)
@pytest.mark.parametrize("layout", ["all_small", "small_mixed"])
def test_small_frames_both_ways(engine, layout, rec_kind):
    """The grid's frames of at most 64 bytes as whole slices of small frames (the all-small
    pipeline) and with a longer frame in every slice (run_class<0, 1, 4>, the LDS transpose)."""
    run_rx(engine, case(layout), rec_kind, f"{layout} REC{rec_kind}")


@pytest.mark.parametrize("layout", ["all_small", "small_mixed"])
def test_small_frames_both_ways_capped(capped_engine, layout):
    """The same with 16 (one workgroup: the two-deep prefetch) or 5-6 slices per wave."""
    run_rx(capped_engine, case(layout), rxg.REC16, f"{layout} capped REC16")


# --------------------------------------------------------------- tx checksum generate ---

def check_tx(eng, frames, what):
    zarena, off, lens = pktgen.pack_arena([cases.zeroed_fields(f) for f in frames])
    want = oracle.tx_batch(zarena, off, lens)
    got = eng.tx_arena(zarena, off, lens)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        i = int(np.searchsorted(off, int(bad[0]) // 64, side="right")) - 1
        raise AssertionError(f"{what}: tx arena differs at {len(bad)} bytes, first in frame {i} "
                             f"({cases.describe(frames[i])}, slice {i // 64}, lane {i % 64}), byte "
                             f"{int(bad[0]) - int(off[i]) * 64}: got {got[bad[0]]:#04x} exp {want[bad[0]]:#04x}")
    # said on its own: nothing but the two fields of each frame changed -- not the bytes at or
    # past data_len, not the 0xA5 slot padding
    field = np.zeros(zarena.size, dtype=bool)
    for o in (24, 25, 50, 51):
        field[off.astype(np.int64) * 64 + o] = True
    assert np.array_equal(got[~field], zarena[~field]), what
    return got


@pytest.mark.parametrize("order", ["grid", "interleaved"])
def test_grid_tx_generate(engine, order):
    """The grid with both checksum fields zeroed through rx_kernel<0>: the oracle's arena byte for
    byte, which is the frames as the Python restatement filled them."""
    c = case(order)
    got = check_tx(engine, c.frames, f"tx {order}")
    assert got.tobytes() == c.arena.tobytes()


def test_grid_tx_generate_capped(capped_engine):
    check_tx(capped_engine, case("interleaved").frames, "tx interleaved capped")


# ------------------------------------------------------------- fused payload hand-off ---

@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16])
@pytest.mark.parametrize("by_ref", [False, True])
def test_grid_fused_payload(engine, by_ref, rec_kind):
    """The interleaved grid through rxg_rx_burst_payload_dev: records, counters, every message
    field, every payload's bytes where its message points (pay_span, pay_writes_chunk,
    pay_line_small over the same (L, total_length) edges).  Copied: the arena, filled with a
    known byte first, holds the pool's bytes in the payloads' 64-byte lines and the fill
    everywhere else (include/rxg.h: other lines are not written)."""
    from oracle import payload as opl
    c = case("interleaved")
    engine.tcb_load(c.tcb, c.live)
    engine.counters_reset()
    recs, pay, msgs, (arena, off, lens) = engine.rx_burst_payload(c.frames, rec_kind, arena_fill=FILL,
                                                                  by_reference=by_ref)
    cnt = engine.counters()
    assert np.array_equal(off, c.off) and np.array_equal(lens, c.lens)  # (the pool as packed: zero padding)
    what = f"fused {'by reference' if by_ref else 'copy'} REC{rec_kind}"
    assert_records(recs, c.want(rec_kind), c.frames, what)
    assert np.array_equal(cnt, c.ecnt), (what, cnt, c.ecnt)
    e_msgs, pays = opl.slots(c.frames, c.exp["c"], c.off)
    for name in ("arena_off", "len", "flags"):
        bad = np.nonzero(msgs[name] != e_msgs[name])[0]
        assert len(bad) == 0, (f"{what}: msgs.{name} differs at {len(bad)} frames, first {int(bad[0])} "
                               f"({cases.describe(c.frames[int(bad[0])])}): got {msgs[name][bad[0]]} "
                               f"exp {e_msgs[name][bad[0]]}")
    npay = sum(p is not None for p in pays)
    assert npay == 4716 and len(pays) == 14964  # the grid's total_lengths in [41, L - 14]
    want = arena.copy() if by_ref else np.full(arena.size, FILL, dtype=np.uint8)
    for i, p in enumerate(pays):
        if p is None:
            continue
        o = int(msgs[i]["arena_off"])
        if pay[o:o + len(p)].tobytes() != p:
            raise AssertionError(f"{what}: payload bytes differ for frame {i} ({cases.describe(c.frames[i])})")
        lo, hi = o & ~63, (o + len(p) + 63) & ~63
        want[lo:hi] = arena[lo:hi]
    if pay.tobytes() != want.tobytes():
        bad = np.nonzero(pay != want)[0]
        i = int(np.searchsorted(c.off, int(bad[0]) // 64, side="right")) - 1
        raise AssertionError(f"{what}: the arena differs at {len(bad)} bytes outside the payloads, first in "
                             f"frame {i} ({cases.describe(c.frames[i])}) at byte {int(bad[0]) - int(c.off[i]) * 64}")


# ------------------------------------------------------------------------ served path ---

@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16])
def test_grid_served(rec_kind):
    """Per class, bursts of the interleaved grid through the resident server (default
    placement): up to 4096 frames, and 64 and 128 frames, which one workgroup's four waves share
    (the cooperative part / parts rounds).  Served == launched == oracle, burst by burst, and the
    counters of the whole sequence equal the launched ones."""
    c = case("interleaved")
    eng = rxg.Engine(device=0, max_batch=1 << 16, max_bytes=64 << 20)
    bufs = []
    try:
        eng.tcb_load(c.tcb, c.live)
        d_arena, d_off, d_len = eng.to_device(c.arena), eng.to_device(c.off), eng.to_device(c.lens)
        cls = np.array([cases.class_of(len(f)) for f in c.frames])
        bursts = []
        for k in range(len(cases.CLASSES)):
            idx = np.nonzero(cls == k)[0]
            first, count = int(idx[0]), len(idx)
            assert count == idx[-1] - idx[0] + 1  # the class's frames are contiguous
            bursts.append((first, min(count, 4096)))
            if count >= 64 + 128:
                bursts += [(first + count - 64, 64), (first + count - 192, 128)]
        total = sum(k for _, k in bursts)
        at = np.concatenate([[0], np.cumsum([k for _, k in bursts])])  # each burst's place in ref / out
        ref, out = eng.alloc(total * rec_kind), eng.alloc(total * rec_kind)
        bufs = [d_arena, d_off, d_len, ref, out]

        def run(burst_fn, dst):
            for (first, k), a in zip(bursts, at):
                burst_fn(d_arena.ptr, d_off.ptr + 4 * first, d_len.ptr + 2 * first, k, dst.ptr + int(a) * rec_kind, rec_kind)
        eng.counters_reset()
        run(eng.rx_burst_dev, ref)
        eng.sync()
        lcnt = eng.counters()
        launched = ref.download(rxg.rec_dtype(rec_kind), total)
        eng.counters_reset()
        eng.sync()
        # Nothing is queued on the context's stream while the server is resident (as in
        # test_gpu_server): the counters are reset before it starts, and they and the records
        # are read once it has stopped.
        eng.server_start(rec_kind, max_frames=4096)
        try:
            run(eng.server_burst_dev, out)
        finally:
            eng.server_stop()
        served = out.download(rxg.rec_dtype(rec_kind), total)
        for (first, k), a in zip(bursts, at):
            what = f"served REC{rec_kind} burst of {k} at {first}"
            fr, got = c.frames[first:first + k], served[a:a + k]
            assert_records(got, launched[a:a + k], fr, what + " against launched", first)
            assert_records(got, c.want(rec_kind, first, first + k), fr, what + " against the oracle", first)
        assert eng.counters().tolist() == lcnt.tolist(), f"served REC{rec_kind}"
        assert int(lcnt[0]) == total
    finally:
        for d in bufs:
            d.free()
        eng.close()


# --------------------------------------------------------------------------- flip set ---

@pytest.mark.parametrize("shorten", [0, 40])
def test_flip_set(engine, shorten):
    """Every byte of a frame of each class counted once and only once: bit-exact with the oracle,
    and the three rules of rxspan_cases.check_flip_rules on the GPU's own records, so the test
    stands even if the oracle shares a misreading."""
    c = case(f"flip{shorten}")
    got = run_rx(engine, c, rxg.REC16, f"flip set (total_length - {shorten})")
    cases.check_flip_rules(c.frames, c.base_of, got, shorten)


# ------------------------------------------------------------------------ extreme set ---

@pytest.mark.parametrize("rec_kind", [rxg.REC16, rxg.REC48])
def test_extreme_set(engine, rec_kind):
    """The largest sums the lane accumulators and group_sum<64> meet (0xFF from byte 34 to the
    end of 9018- and 65535-byte frames), all-zero bodies, and stored checksums of 0x0000 with
    0xFFFF in their place: both representations verify."""
    c = case("extreme")
    got = run_rx(engine, c, rec_kind, f"extreme REC{rec_kind}")
    r = got["c"] if rec_kind == rxg.REC48 else got
    for i, k in enumerate(c.kinds):
        assert r["ip_cksum"][i] == 0, (k, cases.describe(c.frames[i]))
        if k != "fill":
            assert r["tcp_cksum"][i] == 0, (k, cases.describe(c.frames[i]))


def test_extreme_set_tx(engine):
    check_tx(engine, case("extreme").frames, "tx extreme")
