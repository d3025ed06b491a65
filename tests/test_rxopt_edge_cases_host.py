"""CPU: the edge sets of tests/rxopt_edge_cases.py held to what they claim -- which lengths,
data_off nibbles, lanes, verdicts, round counts and (O, p, l) triples occur, both outcomes of the
three bad-length tests at every O, that at every length the poison behind a cut frame would
change the model's answer were it read -- and every frame of every set sent through
the library's host parser (rxg_rx_opt_parse) and compared with the model tests/rxopt_ref.py in
every field, so that model, host parser and (tests/test_gpu_rxopt_edges.py) kernel agree three
ways."""
import numpy as np
import pytest

import rxg
import rxopt_cases as cases
import rxopt_edge_cases as ec
import rxopt_ref as ref
import txreset_cases as tc

FLAGS = ref.FIELDS.index("flags")
FOUND_BITS = (rxg.O_MSS, rxg.O_WSCALE, rxg.O_SACK_PERM, rxg.O_SACK, rxg.O_TS, rxg.O_OTHER)


def slices(seq):
    return [seq[s:s + ec.SLICE] for s in range(0, len(seq), ec.SLICE)]


# ------------------------------------------------------------------ 0. frames and pools ---
def test_frames_pools_and_the_cached_model():
    f = ec.frame(15, ec.BODY_B, 130)
    assert len(f) == 130 and f[46] >> 4 == 15 and f[46] & 0xF and f[54:94] == ec.BODY_B
    assert f[94:130] == bytes(cases.POISON[(j - 54) % 16] for j in range(94, 130))
    assert ec.frame(3, ec.BODY_A, 47)[46] >> 4 == 3 and len(ec.frame(9, b"", 0)) == 0
    # the cache key holds all the rule reads: the model through it is rxopt_ref.records
    for name in ("verdicts", "rounds", "aligned_edges", "len_grid_long"):
        c = ec.get(name)
        assert np.array_equal(c.want, ref.records(c.frames, c.verdicts)), name
    # both layouts: every frame's bytes at its offset, the poison in the frame's phase behind them
    c = ec.get("len_grid_long")
    for arena, off, lens in (c.packed(), c.strided()[:3]):
        assert lens.tolist() == [len(f) for f in c.frames]
        for i in (0, 1, 2, 95, 190, 191):
            o, n = int(off[i]) * 64, len(c.frames[i])
            end = (n + 63) // 64 * 64
            assert arena[o:o + n].tobytes() == c.frames[i]
            assert arena[o + n:o + end].tobytes() == bytes(cases.POISON[(j - 54) % 16] for j in range(n, end))
    arena, off, lens = ec.get("aligned_edges").packed()
    assert len(arena) == (int(off[-1]) + (int(lens[-1]) + 63) // 64) * 64      # the pool ends with the last line
    # the records the sets upload carry the verdicts, in all three layouts
    c = ec.get("verdicts")
    for kind in (rxg.REC8, rxg.REC16, rxg.REC48):
        a, b = c.recs(kind, 0), c.recs(kind, 1)
        assert np.array_equal(tc.verdict_of(a, kind), c.verdicts) and np.array_equal(tc.verdict_of(b, kind), c.verdicts)
        assert not np.array_equal(a, b)


# --------------------------------------------------------------------------- 1. len_grid ---
def test_len_grid_holds_every_length_nibble_and_lane():
    c = ec.get("len_grid")
    assert c.n == ec.LANE_BLOCK + 131 * 16 * len(ec.BODIES) and {"A", "B", "C"} < set(ec.BODIES) and np.isin(c.verdicts, ec.CAND).all()
    grid, gmeta = c.frames[ec.LANE_BLOCK:], c.meta[ec.LANE_BLOCK:]
    assert set(gmeta) == {(ln, d, b) for ln in range(131) for d in range(16) for b in ec.BODIES}
    for f, (ln, d, b) in zip(grid, gmeta):
        assert len(f) == ln and (ln <= 46 or f[46] >> 4 == d) and f[54:94] == ec.BODIES[b][:max(0, ln - 54)]
    for s in slices(gmeta)[:-1]:              # slices mix lengths and data offsets
        assert len({m[0] for m in s}) >= 32 and len({m[1] for m in s}) >= 8 and {m[2] for m in s} == set(ec.BODIES)
    # the chunk-5 test: O = 28, 32, 36 and 40 on both sides of len 80 / 81
    for d in (12, 13, 14, 15):
        for b in ec.BODIES:
            assert not ec.is_far(grid[gmeta.index((80, d, b))]) and ec.is_far(grid[gmeta.index((81, d, b))])
    assert not ec.is_far(grid[gmeta.index((130, 11, "A"))])
    # the lane block
    block = slices(c.frames[:ec.LANE_BLOCK])
    for lane, s, m in zip(ec.LANES, block, slices(c.meta)):
        assert [k for k, f in enumerate(s) if ec.is_far(f)] == [lane]
        assert {"near", "short", "low"} <= set(m)
        for f, what in zip(s, m):
            assert what == ("far" if ec.is_far(f) else "short" if len(f) < 54 else "near" if ec.opt_len(f) > 26 else "low")
            assert what != "near" or len(f) <= 80
            assert what != "low" or (len(f) > 80 and ec.opt_len(f) <= 24)
    assert all(ec.is_far(f) for f in block[len(ec.LANES)]) and len(block) == len(ec.LANES) + 1
    assert {ec.opt_len(f) for f in block[-1]} == {28, 32, 36, 40}


def test_len_grid_outcomes():
    c = ec.get("len_grid")
    flags = [ec.model(f)[FLAGS] for f in c.frames]
    for bit in FOUND_BITS + (rxg.O_CUT, rxg.O_BAD_DOFF, rxg.O_MALFORMED):
        assert any(x & bit for x in flags), bit
    assert any(not x & rxg.O_CUT for x in flags)
    # the frames of exactly 92 bytes whose option bytes 38..39 matter: body B under O = 40
    f92, f96 = ec.frame(15, ec.BODY_B, 92), ec.frame(15, ec.BODY_B, 96)
    assert f92 in c.frames and f96 in c.frames
    m92, m96 = dict(zip(ref.FIELDS, ec.model(f92))), dict(zip(ref.FIELDS, ec.model(f96)))
    assert m96["tsecr"] == 0xD1D2D3D4 and m92["tsecr"] == 0xD1D20000 and m92["tsval"] == m96["tsval"] == 0xC1C2C3C4
    # every length 92..95 differs from the whole frame, so the guard's bound is pinned from both sides
    assert len({ec.model(ec.frame(15, ec.BODY_B, n)) for n in (91, 92, 93, 94, 95)}) == 4
    long = ec.get("len_grid_long")
    assert {m for m in long.meta if m[0] > 130} == {(ln, d, b) for ln in ec.LONG_LENS for d in range(16) for b in ec.BODIES}
    assert all(len(f) == m[0] for f, m in zip(long.frames, long.meta))
    assert all(len({min(m[0], 200) for m in s}) >= 20 for s in slices(long.meta))


def without_cut(rec):
    return rec[:FLAGS] + (rec[FLAGS] & ~rxg.O_CUT,)       # the kernel sets CUT from len alone


def test_poison_behind_a_cut_would_change_the_answer_at_every_length():
    """At every len 0..93 the grid has a frame whose record changes when the bytes at and past len
    hold the poison of its slot instead of reading zero, and at every len whose first missing byte
    the rule reads (46, 54..93) one whose record changes with that single byte.  Per length, not
    per frame: a cut that lands on a length byte is MALFORMED with a zero and with the poison, and
    the poison's two no-operations before a zero end the walk as the zero does."""
    c = ec.get("len_grid")
    whole, single = set(), set()
    for f, (ln, d, b) in zip(c.frames[ec.LANE_BLOCK:], c.meta[ec.LANE_BLOCK:]):
        if ln >= 94 or d != 15:
            continue
        a = without_cut(ec.model(f))
        assert ec.model(f)[FLAGS] & rxg.O_CUT
        if a != without_cut(ec.model(f + ec.poison(128 - ln, ln).tobytes())):
            whole.add(ln)
        if a != without_cut(ec.model(f + ec.poison(1, ln).tobytes())):
            single.add(ln)
    assert whole == set(range(94))
    assert single == {46} | set(range(54, 94))
    # the pools hold exactly that poison behind a frame (test_frames_pools_and_the_cached_model)


# --------------------------------------------------------------------------- 2. verdicts ---
def test_verdicts_puts_every_verdict_on_every_lane():
    c = ec.get("verdicts")
    assert c.n == 6 * ec.SLICE and c.frames[:ec.SLICE] * 6 == c.frames and len(set(c.frames[:ec.SLICE])) == ec.SLICE
    assert {(i % ec.SLICE, int(v)) for i, v in enumerate(c.verdicts)} == {(k, v) for k in range(ec.SLICE) for v in range(6)}
    cand = np.isin(c.verdicts, ec.CAND)
    assert {len(f) for f, x in zip(c.frames, cand) if x} >= {0, 1, 46, 47, 53, 54}
    assert not c.want[~cand].view(np.uint8).any() and (c.want["flags"][cand] & rxg.O_PARSED).all()
    for ln in (0, 1, 46):          # frame[46] is past the frame: BAD_DOFF with O = 0
        i = next(i for i, f in enumerate(c.frames) if len(f) == ln and cand[i])
        assert ref.as_tuple(c.want[i]) == (0, 0, 0, 0, 0, 0, 0, rxg.O_PARSED | rxg.O_BAD_DOFF | rxg.O_CUT)
    for ln in (47, 53):            # data_off 15 is there, no option byte is
        i = next(i for i, f in enumerate(c.frames) if len(f) == ln and cand[i])
        assert ref.as_tuple(c.want[i]) == (0, 0, 0, 0, 0, 0, 40, rxg.O_PARSED | rxg.O_CUT)
    kinds = {(ec.walk(f)[0] > 0, ec.opt_len(f) > 0) for f in c.frames[:ec.SLICE]}
    assert kinds == {(True, True), (False, True), (False, False)}


# ----------------------------------------------------------------------------- 3. rounds ---
def test_rounds_holds_every_round_count_and_layout():
    c = ec.get("rounds")
    s = slices(c.frames)
    m = [x[0] for x in slices(c.meta)]
    v = slices(c.verdicts.tolist())
    count = [[ec.walk(f)[0] for f in x] for x in s]
    assert m == ["base"] + ["permuted"] * 4 + ["one_round"] * 4 + ["never"] * 4 + ["non_candidate"] * 4 + ["partial"]
    for r in range(1, 41):
        assert ec.walk(ec.rounds_frame(r, 3))[0] == r
    # the base slice: every count, one slowest lane, a record of its own on every lane that can carry one
    assert count[0] == ec.base_rounds() and set(count[0]) == set(range(1, 41)) and count[0].count(40) == 1
    carried = [ec.model(f) for f, r in zip(s[0], count[0]) if r <= 38]
    assert len(set(carried)) == len(carried) >= 60
    for f, r in zip(s[0], count[0]):      # what lies behind the end of the list is never found
        assert dict(zip(ref.FIELDS, ec.model(f)))["mss"] != 0xDEAD
        used = 40 if r == 1 or r > 37 else r + 9 if r <= 31 else r + 3      # the bytes up to the end of list
        assert (40 - used >= 4) == (bytes([2, 4, 0xDE, 0xAD]) in f[54:94])
    for k, lane in enumerate(ec.EDGE_LANES):
        assert sorted(s[1 + k]) == sorted(s[0]) and count[1 + k].index(40) == lane and count[1 + k].count(40) == 1
        assert np.isin(v[1 + k], ec.CAND).all()
    for k, lane in enumerate(ec.EDGE_LANES):
        one, never, non = count[5 + k], count[9 + k], count[13 + k]
        for x in (one, never, non):
            assert x[lane] == 40
        assert all(r == 1 for j, r in enumerate(one) if j != lane) and np.isin(v[5 + k], ec.CAND).all()
        assert all(r == 0 for j, r in enumerate(never) if j != lane) and np.isin(v[9 + k], ec.CAND).all()
        assert {ec.opt_len(f) for j, f in enumerate(s[9 + k]) if j != lane} == {0, 12}
        assert [j for j, x in enumerate(v[13 + k]) if x in ec.CAND] == [lane]
        assert min(r for j, r in enumerate(non) if j != lane) >= 2     # walkers, were they candidates
    assert len(s[-1]) == 17 and count[-1] == [1] * 16 + [40] and c.n % ec.SLICE == 17


# ----------------------------------------------------------------------- 4. length_tests ---
@pytest.mark.parametrize("size", ec.OPT_SIZES)
def test_length_tests_hold_every_triple_and_both_outcomes(size):
    c = ec.length_tests(size)
    assert set(range(43)) <= set(ec.LENGTH_BYTES) and len(ec.LENGTH_KINDS) == 6
    want_meta = {(size, p, k, ln) for p in range(size - 1) for k in ec.LENGTH_KINDS for ln in ec.LENGTH_BYTES}
    want_meta |= {(size, size - 1, k, None) for k in ec.LENGTH_KINDS}
    assert set(c.meta) == want_meta and len(c.meta) == len(want_meta)
    outcomes = {"no_length": set(), "short": set(), "over": set()}
    found_behind = 0
    for f, (_, p, k, ln) in zip(c.frames, c.meta):
        assert len(f) == 54 + size <= 94 and ec.opt_len(f) == size and f[54:54 + p] == ec.NOP * p and f[54 + p] == k
        assert ln is None or f[55 + p] == ln
        rounds, events, _ = ec.walk(f)
        if not rounds:                      # two no-operations and (8, 10) under O = 12: the shortcut's frame
            assert (size, p, k, ln) == (12, 2, 8, 10)
            continue
        e = events[0]                       # the option under test is the first the walk meets
        assert e[:3] == (p, k, ln) and rounds >= p + 1
        outcomes["no_length"].add(e[3])
        outcomes["short"].add(e[4])
        outcomes["over"].add(e[5])
        rec = dict(zip(ref.FIELDS, ec.model(f)))
        bad = ln is None or ln < 2 or p + ln > size
        assert bool(rec["flags"] & rxg.O_MALFORMED) == bad and e[3:] == (ln is None, ln is not None and ln < 2,
                                                                        ln is not None and ln >= 2 and p + ln > size)
        if not bad and size - p - ln >= 4:  # the MSS behind a taken option is found: a wrong skip shows
            assert rec["flags"] & rxg.O_MSS and rec["mss"] == (997 * size + 43 * p + ln) & 0xFFFF
            found_behind += 1
        if bad and ln is not None and size - p - 2 >= 4:   # the MSS behind a refused one is not
            assert f[56 + p:58 + p] == bytes([2, 4]) and not rec["flags"] & rxg.O_MSS
    assert all(x == {True, False} for x in outcomes.values()), outcomes
    assert found_behind > 0 or size == 4
    # every source-dword phase and every dword of the ten meets a refused length
    bad_at = {p for (_, p, k, ln) in c.meta if ln is not None and (ln < 2 or p + ln > size)}
    assert bad_at == set(range(size - 1))
    # the order mixes: no slice is one (p, kind)
    assert all(len({(m[1], m[2]) for m in s}) >= 16 for s in slices(c.meta)[:-1])


def test_length_tests_size():
    n = sum(ec.length_tests(size).n for size in ec.OPT_SIZES)
    assert 20000 <= n <= 70000


# ------------------------------------------------------------- 5. sack_grid, aligned_edges ---
def test_sack_grid_holds_every_block_count_at_every_offset():
    c = ec.get("sack_grid")
    assert set(c.meta) == {(size, nb, p) for size in ec.OPT_SIZES for nb in (1, 2, 3, 4) for p in range(size - 8 * nb - 1)}
    assert len(c.meta) == len(set(c.meta))
    for f, (size, nb, p) in zip(c.frames, c.meta):
        rec = dict(zip(ref.FIELDS, ec.model(f)))
        assert (rec["opt_len"], rec["nsack"], rec["sack_off"]) == (size, nb, 56 + p) and rec["flags"] & rxg.O_SACK
        assert not rec["flags"] & (rxg.O_MALFORMED | rxg.O_CUT)
        assert bool(rec["flags"] & rxg.O_MSS) == (size - p - 2 - 8 * nb >= 4)
    assert {dict(zip(ref.FIELDS, ec.model(f)))["sack_off"] for f in c.frames} == set(range(56, 87))


def test_aligned_edges_hold_the_neighbours_every_size_and_the_cuts():
    c = ec.get("aligned_edges")
    by = dict(zip(c.meta, c.frames))
    word = int.from_bytes(cases.ALIGNED_TS, "little")
    assert {m for m in by if m[0] == "bit"} == {("bit", j) for j in range(32)}
    for j in range(32):
        f = by[("bit", j)]
        assert ec.opt_len(f) == 12 and len(f) >= 66 and int.from_bytes(f[54:58], "little") ^ word == 1 << j
        assert ec.walk(f)[0] >= 1                        # no shortcut: the frame walks
        rec = dict(zip(ref.FIELDS, ec.model(f)))
        assert (rec["tsval"], rec["tsecr"]) != (int.from_bytes(f[58:62], "big"), int.from_bytes(f[62:66], "big"))
    for size in range(8, 44, 4):
        f = by[("exact", size)]
        assert ec.opt_len(f) == size and f[54:58] == cases.ALIGNED_TS and len(f) >= 54 + size
        rec = dict(zip(ref.FIELDS, ec.model(f)))
        assert (ec.walk(f)[0] == 0) == (size == 12)
        assert bool(rec["flags"] & rxg.O_TS) == (size >= 12) and bool(rec["flags"] & rxg.O_MALFORMED) == (size == 8)
        assert bool(rec["flags"] & rxg.O_MSS) == (size >= 16)
    for n in range(54, 71):
        f = by[("len", n)]
        assert len(f) == n and ec.opt_len(f) == 12
        rec = dict(zip(ref.FIELDS, ec.model(f)))
        assert bool(rec["flags"] & rxg.O_CUT) == (n < 66) and (ec.walk(f)[0] == 0) == (n >= 58)
    assert len({ec.model(by[("len", n)]) for n in range(54, 71)}) >= 10     # the cuts change the answer


# ------------------------------------------------------------------------------- 6. grid ---
def test_grid_pool_and_sizes():
    slots = ec.grid_slots()
    assert len(slots) == len(set(slots)) == ec.POOL_FRAMES == 257 and max(len(f) for f in slots) <= 128
    flags = [ec.model(f)[FLAGS] for f in slots]
    assert sum(bool(x & rxg.O_CUT) for x in flags) > 20 and sum(bool(x & rxg.O_TS) for x in flags) > 20
    assert sum(ec.is_far(f) for f in slots) > 10 and sum(ec.walk(f)[0] == 0 for f in slots) > 20
    assert ec.GRID_SIZES == [255, 256, 257, 511, 512, 513, 769]     # the multiples of 4 and 8 waves x 64, and one
    for n in ec.GRID_SIZES[:3] + [769]:
        g = ec.GridCase(n)
        pool = g.pool()
        assert len(pool) == 257 * 128 and set(g.verdicts.tolist()) == set(range(6))
        for i in (0, 1, n // 2, n - 1):
            f = g.frame(i)
            o = int(g.off[i]) * 64
            assert pool[o:o + len(f)].tobytes() == f and int(g.lens[i]) == len(f)
            assert pool[o + len(f):o + 128].tobytes() == ec.poison(128 - len(f), len(f)).tobytes()
        frames = [g.frame(i) for i in range(n)]
        assert np.array_equal(g.want, ref.records(frames, g.verdicts))
    g = ec.GridCase(769)
    arena, (slot0, stride64) = g.strided()
    for i in (0, 5, 768):
        o = (slot0 + i * stride64) * 64
        assert arena[o:o + 128].tobytes() == g.pool()[int(g.off[i]) * 64:int(g.off[i]) * 64 + 128].tobytes()
    assert len(arena) == (slot0 + 769 * stride64) * 64


def test_grid_large_passes_every_waves_first_slice():
    n = ec.GRID_LARGE
    g = ec.GridCase(n)
    nslices = (n + 63) // 64
    waves = 256 * ec.RESIDENT_WORKGROUPS * 4        # an MI355X: 256 CUs
    assert n == (1 << 20) + 81 and waves == 8192 and 2 * waves <= nslices <= 3 * waves and n % 64 == 17
    assert set(g.slot.tolist()) == set(range(257)) and n * 48 > 1 << 24 and g.want.shape == (n,)
    sample = np.random.default_rng(1).integers(0, n, 2000)
    sample[:3] = (0, n - 82, n - 1)
    frames = [g.frame(int(i)) for i in sample]
    assert np.array_equal(g.want[sample], ref.records(frames, g.verdicts[sample]))
    cand = np.isin(g.verdicts, ec.CAND)
    assert 0.4 < cand.mean() < 0.6 and not g.want[~cand].view(np.uint8).any()


# ------------------------------------------ 7. the host parser equals the model everywhere ---
@pytest.mark.parametrize("name", list(ec.SETS) + ["grid"])
def test_host_parser_equals_the_model(name):
    frames = ec.grid_slots() if name == "grid" else ec.get(name).frames
    for i, f in enumerate(frames):
        wantrec, got = ec.model(f), ref.as_tuple(rxg.rx_opt_parse(f))
        assert got == wantrec, (name, i, len(f), f[46:94].hex(), got, wantrec)
    if name.startswith("length_tests"):      # and the cache is the plain model on the set whose frames all differ
        c = ec.get(name)
        assert np.array_equal(c.want, ref.records(c.frames, c.verdicts))
