"""GPU: pg_gather (csrc/rxg_payload.hip) on the deterministic sets of gather_cases.py, bit-exact
against oracle.payload.gather on the oracle's records, through rxg_payload_gather_dev into an arena
pre-filled with 0xA5 -- so the zero padding of every message's last chunk is observed, and so is
every byte the gather must leave alone: from the end of the last gathered message, across the
capacity, to the end of a 4 096-byte guard.  What the sets cover (every lane and mark of the
wave's run, every tail and shift, the occupancy edges) is asserted on the CPU in
test_gather_cases_host.py.  Nothing here aims at the look-back timeout.
"""
import functools
import types

import numpy as np
import pytest

import gather_cases as gc
import rxg

pytestmark = pytest.mark.gpu

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
FILL, GUARD = 0xA5, 4096


@pytest.fixture(scope="module")
def sets():
    """name (and arguments) -> gather_cases.Case: each set is built, packed and answered by the
    oracle once for the module."""
    occ = gc.occupancy_sets()

    @functools.lru_cache(maxsize=None)
    def get(name, *args):
        if name == "occupancy_sets":
            return gc.Case(*occ[args[0]])
        return gc.Case(*getattr(gc, name)(*args))
    return get


def want_records(c, rec_kind):
    return c.exp if rec_kind == rxg.REC48 else c.exp["c"] if rec_kind == rxg.REC16 else rxg.rec8_pack(c.exp["c"])


def prepare(engine, c, cap, rec_kind=rxg.REC16, n=None):
    """Upload the set and fill the outputs with 0xA5 (the uploads wait on the context's stream).
    The buffers live until release()."""
    n = c.n if n is None else n
    h = types.SimpleNamespace(c=c, cap=cap, rec_kind=rec_kind, n=n, null_arena=False, bufs=[])

    def filled(nbytes):
        d = engine.alloc(nbytes)
        h.bufs.append(d)
        d.upload(np.full(nbytes, FILL, dtype=np.uint8))
        return d
    try:
        for a in (c.arena, c.off, c.lens):
            h.bufs.append(engine.to_device(a))
        h.recs = filled(max(n, 1) * rec_kind)
        h.arena = filled(cap + GUARD)
        h.msgs = filled(max(n, 1) * 16)
        h.used = filled(8)
    except BaseException:
        release(h)
        raise
    return h


def launch(engine, h, stream=None, null_arena=False):
    """Queue the burst and its gather on `stream`; nothing is waited for."""
    da, do, dl = h.bufs[:3]
    h.null_arena = null_arena
    engine.rx_burst_dev(da.ptr, do.ptr, dl.ptr, h.n, h.recs.ptr, h.rec_kind, stream)
    engine.payload_gather_dev(None if null_arena else h.arena.ptr, h.cap, h.msgs.ptr, h.used.ptr, stream)


def issue(engine, c, cap, rec_kind=rxg.REC16, null_arena=False, n=None):
    h = prepare(engine, c, cap, rec_kind, n)
    try:
        launch(engine, h, None, null_arena)
    except BaseException:
        release(h)
        raise
    return h


def release(h):
    for d in h.bufs:
        d.free()
    h.bufs = []


def where(c, i):
    """Frame i by its place: wave, lane, payload, its first and last chunk in the wave's run."""
    first, last, _ = gc.layout(c.msgs["len"])
    return (f"frame {i} (workgroup {i // gc.WORKGROUP}, wave {i // gc.WAVE}, lane {i % gc.WAVE}, payload "
            f"{int(c.msgs['len'][i])} bytes at data_off {c.frames[i][46] >> 4 if len(c.frames[i]) > 46 else '-'}, "
            f"run chunks {int(first[i])}..{int(last[i])})")


def verify(h, what=""):
    """The five assertions, against oracle.payload.gather on the oracle's records."""
    c, cap, n = h.c, h.cap, h.n
    assert n == c.n
    # 1. the records
    recs = h.recs.download(rxg.rec_dtype(h.rec_kind), n)
    assert recs.tobytes() == want_records(c, h.rec_kind).tobytes(), f"{what}: records differ from the oracle's"
    e_msgs, e_bytes, e_used = c.expect(0 if h.null_arena else cap)
    assert e_used == c.full
    # 2. the bytes the burst needs
    used = int(h.used.download(np.uint64, 1)[0])
    assert used == c.full, f"{what}: arena_used {used:#x}, the oracle needs {c.full:#x}"
    # 3. every field of every message
    msgs = h.msgs.download(rxg.PAYLOAD_MSG_DTYPE, n)
    for name in ("arena_off", "len", "flags"):
        bad = np.nonzero(msgs[name] != e_msgs[name])[0]
        assert len(bad) == 0, (f"{what}: msgs.{name} differs at {len(bad)} frames, first {where(c, int(bad[0]))}: "
                               f"got {msgs[name][bad[0]]} exp {e_msgs[name][bad[0]]}")
    # 4. the gathered bytes, padding included (the arena held 0xA5, not zeros)
    got = h.arena.download(np.uint8, cap + GUARD)
    g = len(e_bytes)
    assert g <= cap or h.null_arena
    if h.null_arena:
        g = 0
    if got[:g].tobytes() != e_bytes[:g].tobytes():
        bad = np.nonzero(got[:g] != e_bytes[:g])[0]
        b = int(bad[0])
        took = np.nonzero(e_msgs["len"])[0]
        i = int(took[np.searchsorted(e_msgs["arena_off"][took], b, side="right") - 1])
        at = b - int(e_msgs["arena_off"][i])
        raise AssertionError(f"{what}: arena differs at {len(bad)} bytes, first in {where(c, i)} at byte {at} "
                             f"(chunk {at // 16}, {'padding' if at >= e_msgs['len'][i] else 'payload'}): "
                             f"got {got[b]:#04x} exp {e_bytes[b]:#04x}")
    # 5. nothing else is written: the rest of the arena, past the capacity, the guard
    bad = np.nonzero(got[g:] != FILL)[0]
    assert len(bad) == 0, (f"{what}: {len(bad)} bytes written outside the gathered messages ({g} bytes, capacity "
                           f"{cap}), first at {g + int(bad[0])}")
    return e_msgs


def check_gather_filled(engine, c, cap=None, rec_kind=rxg.REC16, what="", null_arena=False):
    engine.tcb_load(c.tcb, c.live)
    engine.arp_disable()
    cap = c.full if cap is None else cap
    h = issue(engine, c, cap, rec_kind, null_arena=null_arena)
    try:
        engine.sync()
        return verify(h, f"{what} REC{rec_kind} cap {cap}")
    finally:
        release(h)


# ------------------------------------------------------------ each set, at cap = full ---

@pytest.mark.parametrize("rec_kind", KINDS)
def test_shift_tail_grid(engine, sets, rec_kind):
    """Every tail length at every source shift; payloads of 16k - 1, 16k, 16k + 1 bytes around one
    round, one set and two sets of rounds."""
    c = sets("shift_tail_grid")
    msgs = check_gather_filled(engine, c, rec_kind=rec_kind, what="shift_tail_grid")
    assert (msgs["flags"] & rxg.PM_GATHERED).all()


@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16])
@pytest.mark.parametrize("name", ["run_position_grid", "jumbo_lengths", "rule_edges"])
def test_set_at_full_capacity(engine, sets, name, rec_kind):
    c = sets(name)
    msgs = check_gather_filled(engine, c, rec_kind=rec_kind, what=name)
    assert (msgs["flags"] & rxg.PM_GATHERED).sum() == (c.msgs["len"] > 0).sum() >= 8


@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16])
def test_sparse_many_workgroups(engine, sets, rec_kind):
    """71 workgroups of uneven aggregates, six of them 0: the look-back reads predecessors at
    distance 64 and more."""
    check_gather_filled(engine, sets("sparse_many_workgroups", 1), rec_kind=rec_kind, what="sparse(1)")


@pytest.mark.parametrize("rec_kind", KINDS)
@pytest.mark.parametrize("n", gc.OCC_N)
def test_occupancy_sets(engine, sets, n, rec_kind):
    """Waves and workgroups without a candidate, single candidates on lane 0 and lane 63, bursts
    that end one frame short of, at, and one frame past a wave and a workgroup."""
    for name in gc.occupancy_names(n):
        check_gather_filled(engine, sets("occupancy_sets", name), rec_kind=rec_kind, what=name)


# ------------------------------------------------------------------ capacity corners ---

def corner_caps(c):
    """The sizing call, capacities below and at one chunk, one byte short of everything, and cuts
    inside a batch at a payload's start - 1, + 0, + 1 (a probe with a payload before and after it
    in its batch, and one that starts at the 128-chunk mark)."""
    first, _last, _ = gc.layout(c.msgs["len"])
    probes = gc.run_position_probes()
    caps = {"0": 0, "1": 1, "15": 15, "16": 16, "full-1": c.full - 1}
    for tag, p in (("mid", probes[31]), ("mark", next(p for p in probes if first[p] == 128))):
        assert first[p] > 0 and c.msgs["len"][p + 1:p - p % 64 + 64].any()
        for d in (-1, 0, 1):
            caps[f"{tag}{d:+d}"] = int(c.msgs["arena_off"][p]) + d
    return caps


CORNERS = ["0", "1", "15", "16", "full-1", "mid-1", "mid+0", "mid+1", "mark-1", "mark+0", "mark+1"]


@pytest.mark.parametrize("corner", CORNERS)
def test_capacity_corners(engine, sets, corner):
    c = sets("run_position_grid")
    caps = corner_caps(c)
    assert list(caps) == CORNERS
    cap = caps[corner]
    msgs = check_gather_filled(engine, c, cap=cap, what=f"run_position_grid corner {corner}")
    took = (msgs["flags"] & rxg.PM_GATHERED) != 0
    assert (msgs["arena_off"][took] + msgs["len"][took] <= cap).all()
    if cap <= 16:
        # the sizing call, and capacities the first message (three chunks) does not fit -- so none
        # does: every message zero, nothing written (verify has compared the whole arena with the
        # fill), used == full all the same
        assert not took.any() and not msgs["len"].any() and not msgs["arena_off"].any()
    else:
        assert took.any() and not took.all()


def test_capacity_of_one_chunk_takes_one_message(engine, sets):
    """rule_edges' first candidate is one byte: at a capacity of 16 it alone is gathered."""
    msgs = check_gather_filled(engine, sets("rule_edges"), cap=16, what="rule_edges")
    assert ((msgs["flags"] & rxg.PM_GATHERED) != 0).sum() == 1 and msgs["len"].sum() == 1


# ------------------------------------------------------------------------- arguments ---

def test_null_arena_sizes(engine, sets):
    """arena NULL with arena_cap 0: the sizing call."""
    c = sets("run_position_grid")
    msgs = check_gather_filled(engine, c, cap=0, what="NULL arena", null_arena=True)
    assert not msgs["flags"].any()


def test_null_arena_with_capacity_is_refused(engine, sets):
    """arena NULL with arena_cap 16: -EINVAL with the binding's message, and nothing is queued --
    the outputs keep their fill."""
    c = sets("rule_edges")
    engine.tcb_load(c.tcb, c.live)
    engine.arp_disable()
    h = issue(engine, c, 0)
    try:
        engine.sync()
        for d in (h.msgs, h.used):
            d.upload(np.full(d.nbytes, FILL, dtype=np.uint8))
        with pytest.raises(rxg.RxgError, match=r"\(-22\): rxg_payload_gather_dev: NULL output buffer"):
            engine.payload_gather_dev(None, 16, h.msgs.ptr, h.used.ptr)
        engine.sync()
        assert (h.msgs.download(np.uint8, h.msgs.nbytes) == FILL).all()
        assert (h.used.download(np.uint8, 8) == FILL).all()
        # the burst is still there to gather
        engine.payload_gather_dev(None, 0, h.msgs.ptr, h.used.ptr)
        engine.sync()
        assert int(h.used.download(np.uint64, 1)[0]) == c.full
    finally:
        release(h)


def test_empty_burst_leaves_used_zero(engine, sets):
    """n = 0: no launch; arena_used is 0, the arena and the messages are not written."""
    c = sets("rule_edges")
    engine.tcb_load(c.tcb, c.live)
    h = issue(engine, c, 64, n=0)
    try:
        engine.sync()
        assert int(h.used.download(np.uint64, 1)[0]) == 0
        assert (h.arena.download(np.uint8, 64 + GUARD) == FILL).all()
        assert (h.msgs.download(np.uint8, 16) == FILL).all()
    finally:
        release(h)


# -------------------------------------------------------- reuse across launches ---

def test_reuse_across_launches_on_one_context(sets):
    """Status words are epoch-tagged, tickets count across launches, the status buffer is cleared
    only when it grows.  On a fresh context: a small first gather (a small status buffer), one of
    71 workgroups (the buffer grows), a one-frame burst, 71 workgroups again (every slot holds a
    word of an older epoch), then six workgroups -- each step checked in full."""
    steps = [("occupancy_sets", "n65_lane0"), ("sparse_many_workgroups", 1), ("occupancy_sets", "n1_single_first"),
             ("sparse_many_workgroups", 2), ("run_position_grid",)]
    with rxg.Engine(device=0) as eng:
        for k, key in enumerate(steps):
            msgs = check_gather_filled(eng, sets(*key), what=f"reuse step {k + 1} {key}")
            assert (msgs["flags"] & rxg.PM_GATHERED).any()


# -------------------------------------------------------------------- two streams ---

def test_two_gathers_back_to_back_on_two_streams(engine, sets):
    """Two bursts and their gathers queued on two registered streams with no host wait in between,
    each into its own outputs: one gather is in flight per context (the ticket counter and the
    status words are shared), so the second waits for the first on the device."""
    import torch
    a, b = sets("sparse_many_workgroups", 2), sets("run_position_grid")
    assert a.tcb.tobytes() == b.tcb.tobytes()
    engine.tcb_load(a.tcb, a.live)
    engine.arp_disable()
    engine.tcb_sync()
    engine.sync()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        engine.stream_register(s.cuda_stream)
    hs = []
    try:
        hs = [prepare(engine, c, c.full) for c in (a, b)]
        launch(engine, hs[0], s1.cuda_stream)
        launch(engine, hs[1], s2.cuda_stream)
        for s in (s1, s2):
            engine.stream_sync(s.cuda_stream)
        verify(hs[0], "first (71 workgroups, s1)")
        verify(hs[1], "second (6 workgroups, s2)")
    finally:
        for h in hs:
            release(h)
        for s in (s1, s2):
            engine.stream_retire(s.cuda_stream)
