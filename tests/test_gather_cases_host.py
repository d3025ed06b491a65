"""CPU: the payload-gather sets of gather_cases.py cover what they claim.  The GPU tests
(test_gpu_gather_edges.py) compare the kernel with oracle.payload.gather on these sets; here the
sets themselves are checked, through gather_cases.layout (where a payload's chunks fall in a
wave's run) and on the oracle's own candidates: every lane, every mark, every tail and shift, the
empty workgroups where they are meant to be.  And the oracle's arena, re-sliced per message, is
each frame's own bytes, which does not go through the oracle's records.
"""
import functools

import numpy as np
import pytest

import gather_cases as gc
from oracle import payload as opl

OCC = gc.occupancy_sets()


@functools.lru_cache(maxsize=None)
def case(name, *args):
    if name == "occupancy_sets":
        return gc.Case(*OCC[args[0]])
    return gc.Case(*getattr(gc, name)(*args))


def lens_of(c):
    return c.msgs["len"].astype(np.int64)


def check_inputs(c, want, exact=True):
    """A condition on the inputs: the frames meant as candidates are candidates per the oracle
    (at least 95 % of them; here all of them, and no other frame)."""
    got = lens_of(c) > 0
    want = np.asarray(want, dtype=bool)
    assert (got & want).sum() >= 0.95 * want.sum()
    if exact:
        assert np.array_equal(got, want)


def check_own_bytes(c):
    """oracle.payload.gather's arena per message == the frame's bytes [34 + 4 * data_off : + len],
    the padding to 16 bytes zero, the messages packed in packet order with no gap."""
    at = 0
    for i in np.nonzero(c.msgs["flags"] & opl.PM_GATHERED)[0]:
        m = c.msgs[i]
        length, off = int(m["len"]), int(m["arena_off"])
        assert off == at and length > 0
        assert c.bytes[off:off + length].tobytes() == gc.own_bytes(c.frames[i], length), f"frame {i}"
        at = off + 16 * gc.chunks(length)
        assert not c.bytes[off + length:at].any()
        assert int(m["flags"]) == opl.PM_GATHERED | (opl.PM_REF_OVERSIZE if length >= 1000 else 0)
    assert at == c.full == len(c.bytes)
    assert not c.msgs["len"][(c.msgs["flags"] & opl.PM_GATHERED) == 0].any()


def test_layout_rule():
    """The restatement on a hand-worked group: 17 bytes then 1 byte then 16 bytes, a second group."""
    lens = [0, 17, 0, 1, 16] + [0] * 59 + [33]
    first, last, total = gc.layout(lens)
    assert [first[i] for i in (1, 3, 4, 64)] == [0, 2, 3, 0]
    assert [last[i] for i in (1, 3, 4, 64)] == [1, 2, 3, 2]
    assert first[0] == last[0] == -1 and total.tolist() == [4, 3]
    assert gc.aggregates([16] * 1024 + [1]).tolist() == [1024, 1]


def test_shift_tail_grid():
    c = case("shift_tail_grid")
    check_inputs(c, gc.meant("shift_tail_grid"))
    check_own_bytes(c)
    lens = lens_of(c)
    assert set(lens) == set(gc.shift_tail_lengths())
    assert set(range(1, 81)) <= set(lens)
    for k in (8, 62, 63, 64, 90, 127, 128, 129, 255, 256, 257):
        assert {16 * k - 1, 16 * k, 16 * k + 1} <= set(lens)
    cells = {(gc.shift_of(f), int(length) % 16, f[46] >> 4) for f, length in zip(c.frames, lens)}
    assert {(s, t) for s, t, _ in cells} == {(s, t) for s in (6, 10, 14, 2) for t in range(16)}
    assert {d for _, _, d in cells} == set(range(5, 16))
    for length in set(lens):     # every length at every data_off
        assert {f[46] >> 4 for f, x in zip(c.frames, lens) if x == length} == set(range(5, 16))
    assert all(c.frames[i][34 + 4 * (c.frames[i][46] >> 4) + int(lens[i]) - 1] != 0 for i in range(c.n))


def test_run_position_grid():
    c = case("run_position_grid")
    check_inputs(c, gc.meant("run_position_grid"))
    check_own_bytes(c)
    lens = lens_of(c)
    first, last, total = gc.layout(lens)
    probes = gc.run_position_probes()
    assert c.n % 64 == 0 and all(lens[p] > 0 for p in probes)
    assert {int(first[p]) % 64 for p in probes} == set(range(64))
    assert {int(last[p]) % 64 for p in probes} == set(range(64))
    # (also as plain run indices below 64: the first round's lanes)
    assert {int(first[p]) for p in probes} >= set(range(64))
    for m in gc.MARKS:
        assert any(first[p] < m < last[p] for p in probes), f"no probe straddles {m}"
        assert any(first[p] == m for p in probes), f"no probe starts at {m}"
        assert any(last[p] == m - 1 for p in probes), f"no probe ends before {m}"
        # and both where another payload follows in the run, and where the run ends
        assert any(last[p] == m - 1 and total[p // 64] == m for p in probes)
        assert any(last[p] == m - 1 and total[p // 64] > m for p in probes)
    assert any(first[p] < 64 and last[p] > 256 for p in probes)
    assert set(gc.EXACT_T) <= set(total.tolist())
    groups = lens.reshape(-1, 64)
    assert any((g == 1).all() for g in groups)                                   # 64 one-byte payloads
    assert any((g > 0).sum() == 1 and g.max() == gc.MAX_PAYLOAD for g in groups)  # one maximal payload
    assert len(c.frames[int(np.argmax(lens))]) == gc.MAX_FRAME
    # both fillers and candidates on lane 0 and on lane 63 of some batch
    assert {bool(g[0]) for g in groups} == {bool(g[63]) for g in groups} == {False, True}


def test_jumbo_lengths():
    c = case("jumbo_lengths")
    check_inputs(c, gc.meant("jumbo_lengths"))
    check_own_bytes(c)
    lens = lens_of(c)
    cells = {(int(lens[i]), c.frames[i][46] >> 4) for i in range(c.n) if lens[i] > 1}
    assert cells == {(4095, 5), (4096, 5), (4097, 5), (9000, 5), (65481, 5), (9000, 15), (65441, 15)}
    assert cells == set(gc.jumbo_cells())
    assert max(len(f) for f in c.frames) == 65535
    assert sum(len(f) == 65535 for f in c.frames) == 4      # both data_offs, each twice
    for i in np.nonzero(lens > 1)[0]:                      # the follower, in the same batch
        assert lens[i + 1] == 1 and i // 64 == (i + 1) // 64
    assert ((lens.reshape(-1, 64) > 1).sum(axis=1)).tolist() == [1] * 7 + [7]


@pytest.mark.parametrize("n", gc.OCC_N)
def test_occupancy_sets(n):
    names = gc.occupancy_names(n)
    want_names = {"lane0", "lane63", "single_first", "single_last", "one_wave"}
    if n > 1024:
        want_names |= {"single_1024", "first_wg_empty", "last_wg_empty"}
    if n > 2048:
        want_names |= {"middle_wg_empty"}
    assert {x.split("_", 1)[1] for x in names} == want_names
    meant = gc.meant("occupancy_sets")
    for name in names:
        c = case("occupancy_sets", name)
        assert c.n == n
        check_inputs(c, meant[name])
        check_own_bytes(c)
        lens = lens_of(c)
        idx = np.nonzero(lens)[0]
        agg = gc.aggregates(lens)
        waves = {int(i) // 64 for i in idx}
        nwave, nwg = (n + 63) // 64, (n + 1023) // 1024
        assert set(lens[idx]) <= set(gc.OCC_LENGTHS)
        kind = name.split("_", 1)[1]
        if kind == "lane0":
            assert idx.tolist() == list(range(0, n, 64))
        elif kind == "lane63":
            assert idx.tolist() == list(range(63, n, 64))
        elif kind.startswith("single"):
            assert idx.tolist() == [{"single_first": 0, "single_last": n - 1, "single_1024": 1024}[kind]]
        elif kind == "one_wave":
            assert waves == {nwave // 2} and len(idx) == min(64, n - 64 * (nwave // 2))
        elif kind == "first_wg_empty":
            assert agg[0] == 0 and (agg[1:] > 0).all()
        elif kind == "last_wg_empty":
            assert agg[-1] == 0 and (agg[:-1] > 0).all()
        else:
            assert kind == "middle_wg_empty" and nwg >= 3
            mid = (nwg - 1) // 2
            assert 0 < mid < nwg - 1 and agg[mid] == 0 and (np.delete(agg, mid) > 0).all()
    # over the n's sets, all six lengths
    assert n < 1023 or {int(x) for nm in names for x in lens_of(case("occupancy_sets", nm))} >= set(gc.OCC_LENGTHS)


def test_occupancy_sets_no_candidate_at_all():
    """n of 1 and 63 with candidates only on lane 63: a burst whose every wave is empty."""
    for n in (1, 63):
        assert not lens_of(case("occupancy_sets", f"n{n}_lane63")).any()


@pytest.mark.parametrize("seed", [1, 2])
def test_sparse_many_workgroups(seed):
    c = case("sparse_many_workgroups", seed)
    check_inputs(c, gc.meant("sparse_many_workgroups", seed))
    check_own_bytes(c)
    assert c.n == 70 * 1024 + 5 and len(set(map(id, c.frames))) <= 64
    lens = lens_of(c)
    ncand = int((lens > 0).sum())
    assert c.n / 60 < ncand < c.n / 25          # about one frame in 40
    agg = gc.aggregates(lens)
    assert len(agg) == 71
    empty = np.nonzero(agg == 0)[0].tolist()
    assert empty == gc.sparse_empty_workgroups(seed) and len(empty) >= 5
    assert all(0 < g < 70 for g in empty) and any(b == a + 1 for a, b in zip(empty, empty[1:]))
    assert len(set(agg.tolist())) > 40          # the aggregates differ
    assert agg[0] > 0 and agg[70] > 0           # the five-frame last workgroup has a payload
    # a wrongly indexed predecessor shows: neighbouring aggregates differ nearly everywhere
    assert (np.diff(agg) != 0).sum() > 60


def test_sparse_seeds_differ():
    a, b = case("sparse_many_workgroups", 1), case("sparse_many_workgroups", 2)
    assert a.full != b.full and not np.array_equal(a.msgs["len"], b.msgs["len"])


def test_rule_edges():
    c = case("rule_edges")
    check_own_bytes(c)
    kinds = gc.rule_edge_kinds()
    rec = c.exp["c"]
    got = lens_of(c) > 0
    assert got.sum() >= 8 and (~got).sum() >= 8
    for kind, (_kw, verdict) in gc.RULE_KINDS.items():
        k = np.array([x == kind for x in kinds])
        full = k & (c.lens >= 54)
        assert (rec["verdict"][full] == verdict).all(), kind
        # the cases, in the builder's order
        dl = rec["datalen"][k].tolist()
        assert dl[:5] == [0, 1, 33, 34, 65535 - 40], kind
        assert (rec["flags"][k][5:7] & opl.F_TRUNC).all() and not (rec["flags"][k][:5] & opl.F_TRUNC).any()
        assert dl[7:9] == [100 - 4, 100 - 40] and dl[9] == 40                   # IHL 6, IHL 15, bad checksum
        assert dl[10:] == [40 + 4 * (5 - d) for d in range(5)]                  # data_off 0..4
        assert rec["tcp_cksum"][k][9] != 0 or verdict == 3
        cand = got[k].tolist()
        if verdict <= opl.V_RST_LISTEN_NONSYN:
            assert cand == [False, True, True, False, False, False, False, True, True, True] + [True] * 5, kind
        else:
            assert not any(cand), kind
    # IHL 6 / 15 with data_off 5: the bytes are still taken at 34 + 4 * data_off = 54
    i = kinds.index("dispatch") + 7
    for j, length in ((i, 96), (i + 1, 60)):
        m = c.msgs[j]
        assert int(m["len"]) == length
        assert c.bytes[int(m["arena_off"]):int(m["arena_off"]) + length].tobytes() == c.frames[j][54:54 + length]
