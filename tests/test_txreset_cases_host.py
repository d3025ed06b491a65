"""CPU: the reset-build sets of tests/txreset_cases.py hold what they claim.  The GPU tests
(test_gpu_txreset_edges.py) compare the kernels with txreset_cases.build_fast on these sets; here
build_fast is pinned byte for byte to the reference model (txreset_ref.build, itself pinned in
test_txreset_host.py), the hand-written records to their layouts, and every claim of the sets --
forced slices, slice counts, lanes, holes, lengths, where each cap falls, the checksum corners --
is asserted on the masks and lines themselves, not on their names."""
import os
import struct

import numpy as np
import pytest

import oracle
import pktgen
import rxg
import txreset_cases as tc
import txreset_ref as ref

KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]


def same(got, want, what):
    assert got[2] == want[2], (what, "count")
    assert got[1].dtype == want[1].dtype and np.array_equal(got[1], want[1]), (what, "idx")
    assert got[0].dtype == want[0].dtype and got[0].shape == want[0].shape, what
    bad = np.nonzero(got[0] != want[0])[0]
    assert not len(bad), (what, "reset", int(bad[0]) // 64, "byte", int(bad[0]) % 64)


def pin(c, caps, what, n=None):
    n = c.n if n is None else n
    for cap in caps:
        same(tc.build_fast(c.pool, c.off[:n], c.lens[:n], c.verdicts[:n], c.ip_id0, tc.MAC, cap),
             ref.build(c.pool, c.off[:n], c.lens[:n], c.verdicts[:n], c.ip_id0, tc.MAC, cap), f"{what}, cap {cap}")


def slice_view(mask):
    m = np.zeros((len(mask) + tc.SLICE - 1) // tc.SLICE * tc.SLICE, dtype=bool)
    m[:len(mask)] = mask
    return m.reshape(-1, tc.SLICE)


# ------------------------------------------------------------------- 1. the model pin ---
def test_build_fast_equals_the_reference_model_on_the_parity_set():
    rows, frames = pktgen.parity_set(seed=77, n=3000)
    tcb, live = pktgen.table_arrays(rows)
    arena, off, lens = pktgen.pack_arena(frames)
    v = oracle.rx_batch(arena, off, lens, tcb, live)[0]["c"]["verdict"]
    for ip_id0, mac, cap in ((0xFFF0, rxg.REF_SRC_MAC, 1 << 20), (7, tc.MAC, 100), (0, tc.MAC, 0)):
        want = ref.build(arena, off, lens, v, ip_id0, mac, cap)
        assert want[2] > 200
        same(tc.build_fast(arena, off, lens, v, ip_id0, mac, cap), want, f"parity set, cap {cap}")


def test_build_fast_equals_the_reference_model_on_the_small_sets():
    for name, c in tc.rank_cases().items():
        pin(c, [c.n], f"rank {name}")
        s = c.strided(3, 2)
        pin(s, [s.n], f"rank {name}, strided")
        same(s.want(s.n), c.want(c.n), f"rank {name}: the strided pool holds the same frames")
    c = tc.length_case()
    pin(c, [c.n], "lengths")
    # the mask bites, and the poisoned copy differs from the pool only at and past len
    full = tc.build_fast(c.pool, c.off, np.full(c.n, 64), c.verdicts, 0, tc.MAC, c.n)
    assert full[0].tobytes() != c.want(c.n)[0].tobytes()
    p, d = c.pool.reshape(-1, 64), c.dev_pool.reshape(-1, 64)
    for i in range(c.n):
        ln = min(int(c.lens[i]), 64)
        assert np.array_equal(p[i, :ln], d[i, :ln]) and (d[i, ln:] == 0xFF).all() and not (p[i] == 0xFF).any()
    c = tc.cap_case()
    pin(c, tc.caps(), "cap")
    for r in range(len(tc.CORNER_KINDS)):
        c = tc.corner_case(r)
        pin(c, [c.n], f"corners, rotation {r}")


def test_build_fast_equals_the_reference_model_on_the_head_of_a_scan_case():
    nslices = 16384 + 1025
    c = tc.scan_case(nslices, tc.scan_n(nslices)[0])
    c.ip_id0 = 0xFFF0
    pin(c, [20000], "scan head", n=20000)
    assert c.verdicts[:20000].size == 20000 and np.isin(c.verdicts[:20000], tc.RST).sum() > 1000


# -------------------------------------------------------------- 2. the record helpers ---
@pytest.mark.parametrize("rec_kind", KINDS)
def test_records_carry_the_verdicts_and_random_bits_elsewhere(rec_kind):
    v = np.random.default_rng(3).integers(0, 6, 5000).astype(np.uint8)
    a, b = tc.make_recs(v, rec_kind, 1), tc.make_recs(v, rec_kind, 2)
    assert a.dtype == np.uint8 and a.size == v.size * rec_kind
    assert np.array_equal(tc.verdict_of(a, rec_kind), v) and np.array_equal(tc.verdict_of(b, rec_kind), v)
    assert np.array_equal(tc.verdict_of(a.view(rxg.rec_dtype(rec_kind)), rec_kind), v)
    # the layouts of include/rxg.h, through the package's own views of them
    if rec_kind == rxg.REC8:
        assert np.array_equal(rxg.rec8_expand(a.view(rxg.REC8_DTYPE))["verdict"], v)
    else:
        r = a.view(rxg.rec_dtype(rec_kind))
        assert np.array_equal((r["c"] if rec_kind == rxg.REC48 else r)["verdict"], v)
    # every bit outside the verdict field takes both values, and differs between two seeds
    bits_a = np.unpackbits(a.reshape(-1, rec_kind), axis=1, bitorder="little")
    bits_b = np.unpackbits(b.reshape(-1, rec_kind), axis=1, bitorder="little")
    field = np.zeros(rec_kind * 8, dtype=bool)
    if rec_kind == rxg.REC8:
        field[24:27] = True
    else:
        field[64:72] = True
    free = ~field
    assert bits_a[:, free].any(axis=0).all() and (~bits_a[:, free].astype(bool)).any(axis=0).all()
    assert (bits_a[:, free] != bits_b[:, free]).any(axis=0).all()
    assert np.array_equal(bits_a[:, field], bits_b[:, field])
    # the neighbours the kernel's mask and shift must leave out: REC8 bits 23 and 27, bytes 9-11
    if rec_kind == rxg.REC8:
        w0 = a.view("<u4")[::2]
        assert {0, 1} == set(((w0 >> 23) & 1).tolist()) == set(((w0 >> 27) & 1).tolist())
    else:
        assert all(len(set(a.reshape(-1, rec_kind)[:, k].tolist())) > 200 for k in (9, 10, 11))


def test_verdicts_for_uses_all_six_values():
    m = np.random.default_rng(0).random(4000) < 0.3
    v = tc.verdicts_for(m, 4)
    assert set(v.tolist()) == set(range(6))
    assert np.array_equal(np.isin(v, ref.RST_VERDICTS), m)


# ----------------------------------------------------------- 3. the claims of the sets ---
def test_geometry_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(rxg.__file__))), "csrc", "rxg_txreset.hip")).read()
    assert "constexpr uint32_t kScanLanes = 1024, kScanPer = 16;" in src
    assert "const uint32_t i = s * 64u + lane;" in src and "for (uint32_t r = 0; r < cnt; r += 16u)" in src
    assert (tc.SLICE, tc.SCAN_PER, tc.SCAN_WAVE, tc.SCAN_ROUND, tc.BUILD_ROUND) == (64, 16, 64 * 16, 1024 * 16, 16)


def test_scan_sizes_are_the_edges_of_lane_wave_and_round():
    assert tc.SCAN_NSLICES == [15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 16384 + 1025, 2 * 16384 + 17]
    for unit in (tc.SCAN_PER, tc.SCAN_WAVE, tc.SCAN_ROUND):
        assert {unit - 1, unit, unit + 1} <= set(tc.SCAN_NSLICES)
    assert max(tc.scan_n(max(tc.SCAN_NSLICES))) == 2098240
    assert tc.STALE_FIRST > tc.SCAN_ROUND and all(s % tc.SCAN_PER for s in tc.STALE_THEN)


@pytest.mark.parametrize("nslices", tc.SCAN_NSLICES)
def test_scan_case_has_its_forced_slices_and_its_mean(nslices):
    total = {}
    for n in tc.scan_n(nslices):
        c = tc.scan_case(nslices, n)
        assert c.n == n and (n + tc.SLICE - 1) // tc.SLICE == nslices
        per = slice_view(c.mask).sum(axis=1)
        frames = np.minimum(n - tc.SLICE * np.arange(nslices), tc.SLICE)
        assert frames[-1] == (tc.SLICE if n % tc.SLICE == 0 else 1)
        forced = np.zeros(nslices, dtype=bool)
        for unit in (tc.SCAN_PER, tc.SCAN_WAVE, tc.SCAN_ROUND):
            first, last = np.arange(0, nslices, unit), np.arange(unit - 1, nslices, unit)
            assert len(first) and np.array_equal(per[first], np.minimum(64, frames[first])), unit
            assert np.array_equal(per[last], np.ones(len(last))), unit
            forced[first] = forced[last] = True
        if nslices >= tc.SCAN_PER:
            assert (per == 64).any() and (per == 1).any()
        # the slices that are not forced: sparse, and in the larger sizes of every free count
        free = per[~forced]
        if nslices > 1000:
            assert free.mean() <= tc.FREE_MEAN_MAX and per.mean() <= 4.5
        if nslices > 16000:
            assert set(tc.FREE_COUNTS.tolist()) <= set(free.tolist())
        total[n] = int(per.sum())
        # seeded lanes: in a slice of two to five resets every lane is used somewhere
        if nslices > 16000:
            few = slice_view(c.mask)[(per >= 2) & (per <= 5)]
            assert few.any(axis=0).all()
        assert set(c.verdicts.tolist()) == set(range(6)) or nslices < 100
        assert c.off.max() < tc.POOL_LINES and set(c.lens.tolist()) == set(tc.SCAN_LENS.tolist())
    assert max(total.values()) * 64 < 10e6   # what comes back from the largest case, in bytes


def test_scan_cases_reach_the_later_waves_and_the_second_and_third_round():
    """What the sizes are for: resets whose base comes through wsum[] (a slice past 1 024), through
    `carry` (a slice past 16 384, and past 32 768), and a reset in the very last slice."""
    for nslices in tc.SCAN_NSLICES:
        for n in tc.scan_n(nslices):
            per = slice_view(tc.scan_case(nslices, n).mask).sum(axis=1)
            assert per[-1] >= 1 and per[0] >= 1
            for edge in (tc.SCAN_WAVE, tc.SCAN_ROUND, 2 * tc.SCAN_ROUND):
                if nslices > edge:
                    assert per[edge:].sum() >= 1 and per[:edge].sum() > 64


def test_flood_case_is_all_resets():
    c = tc.flood_case(tc.STALE_FIRST)
    assert c.n == 64 * tc.STALE_FIRST and c.mask.all() and c.count == c.n


def test_rank_cases_place_what_they_name():
    cases = tc.rank_cases()
    assert set(cases) == {"low", "high", "spread", "holes", "single", "last1", "last63"}
    assert tc.RANK_COUNTS == [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
    lanes = np.arange(64)
    for name in ("low", "high", "spread"):
        m = slice_view(cases[name].mask)
        assert m.sum(axis=1).tolist() == tc.RANK_COUNTS
        for row, cnt in zip(m, tc.RANK_COUNTS):
            on = lanes[row]
            if name == "low":
                assert on.tolist() == list(range(cnt))
            elif name == "high":
                assert on.tolist() == list(range(64 - cnt, 64))
            elif cnt > 1:
                assert on[0] == 0 and on[-1] == 63 and np.diff(on).max() <= 64 // (cnt - 1) + 1
            else:
                assert 0 < on[0] < 63
    m = slice_view(cases["holes"].mask)
    assert [lanes[~row].tolist() for row in m] == [[0], [31], [32], [63]]
    m = slice_view(cases["single"].mask)
    assert m.shape == (64, 64) and all(lanes[row].tolist() == [s] for s, row in enumerate(m))
    for tail in (1, 63):
        c = cases[f"last{tail}"]
        assert c.n % 64 == tail and c.mask[-1] and slice_view(c.mask)[-1].sum() == 1
        assert c.mask[:-tail].sum() > 10
    for c in cases.values():
        assert 64 <= c.n <= 4096 and set(c.verdicts[c.mask].tolist()) == set(ref.RST_VERDICTS)


def test_length_case_has_every_length_among_its_resets():
    c = tc.length_case()
    assert tc.LENGTHS == list(range(65)) + [65, 1514, 65535]
    assert set(c.lens[c.mask].tolist()) == set(tc.LENGTHS)
    assert (~c.mask).any() and len(set(c.off.tolist())) == c.n
    # every length at every one of the four lanes of a group that loads (the reset's rank mod 4
    # does not matter: lane c of any group loads chunk c), and on both sides of a 16-reset round
    rank = np.cumsum(c.mask) - 1
    assert {0, 15, 16} <= set((rank[c.mask] % 32).tolist())


def test_every_cap_lands_where_it_says():
    c = tc.cap_case()
    per = slice_view(c.mask).sum(axis=1)
    assert per.tolist() == [64, 0, 17, 64, 5]
    base = np.concatenate([[0], np.cumsum(per)])
    caps = tc.caps()
    assert caps == sorted(set(caps)) and caps[0] == 0 and caps[-1] == c.count + tc.GUARD
    for s, cnt in enumerate(per):
        assert {int(base[s]), int(base[s]) + 1, int(base[s]) + int(cnt)} <= set(caps), s
    # inside the first full slice: below, on and above a round's edge, so that groups of one
    # round differ in `act`, and the edge of the last round
    assert per[0] == 64 and {15, 16, 17, 31, 32, 33, 48, 63} <= set(caps)
    # and inside the second full slice (base 81, no multiple of 16: the edge falls inside a round)
    assert per[3] == 64 and base[3] % 16 and {int(base[3]) + 1} <= set(caps)
    for cap in caps:
        want = c.want(cap)
        assert want[2] == c.count and len(want[1]) == min(cap, c.count)


# ------------------------------------------------------------- 4. the checksum corners ---
def fold_once(s):
    return (s & 0xFFFF) + (s >> 16)


@pytest.mark.parametrize("ip_id", [0, 1, 0x00FF, 0xFF00, 0xFFF0, 0xFFFF])
def test_corner_offenders_reach_their_corners(ip_id):
    one = lambda kind: ref.one(tc.corner_offender(kind, ip_id), ip_id, tc.MAC)
    for kind in ("ip", "both"):
        r = one(kind)
        assert r[24:26] == b"\0\0", kind
        assert oracle.calculate_checksum(r[14:24] + b"\0\0" + r[26:34]) == 0
        assert pktgen.py_checksum(r[14:24] + b"\0\0" + r[26:34]) == 0
        assert sum(tc.ip_words(r)) % 0xFFFF == 0 and sum(tc.ip_words(r)) > 0
    for kind in ("tcp", "both"):
        r = one(kind)
        pseudo = r[26:34] + b"\x00\x06" + (20).to_bytes(2, "big")
        assert r[50:52] == b"\0\0", kind
        assert oracle.calculate_checksum(pseudo + r[34:50] + b"\0\0" + r[52:54]) == 0
        assert pktgen.py_checksum(pseudo + r[34:50] + b"\0\0" + r[52:54]) == 0
    assert one("ip")[50:52] != b"\0\0" and one("tcp")[24:26] != b"\0\0"
    # carry: as the kernel adds the words (little-endian, checksum fields zero), one fold is not enough
    r = bytearray(one("carry"))
    r[24:26] = r[50:52] = b"\0\0"
    for words in (tc.ip_words, tc.tcp_words):
        s = sum(tc.swapped(words(r)))
        assert fold_once(s) > 0xFFFF and fold_once(fold_once(s)) <= 0xFFFF
    # zero and ones are what they say
    assert tc.corner_offender("zero", ip_id) == bytes(64) and tc.corner_offender("ones", ip_id) == b"\xff" * 64


def test_all_ones_line_at_id_ffff_has_sums_past_two_folds_worth():
    r = bytearray(ref.one(tc.corner_offender("ones", 0xFFFF), 0xFFFF, tc.MAC))
    assert r[18:20] == b"\xff\xff" and r[26:42] == b"\xff" * 16
    r[24:26] = r[50:52] = b"\0\0"
    for words in (tc.ip_words, tc.tcp_words):
        assert sum(words(r)) > 0x1FFFE and sum(tc.swapped(words(r))) > 0x1FFFE
    # the stored checksums are the complement of the fully folded sums
    full = ref.one(b"\xff" * 64, 0xFFFF, tc.MAC)
    for words, at in ((tc.ip_words, 24), (tc.tcp_words, 50)):
        s = sum(words(r))
        while s >> 16:
            s = fold_once(s)
        assert struct.unpack("!H", full[at:at + 2])[0] == (~s) & 0xFFFF


def test_corner_cases_put_every_kind_on_every_rank():
    seen = set()
    for rot in range(len(tc.CORNER_KINDS)):
        c = tc.corner_case(rot)
        per = slice_view(c.mask).sum(axis=1)
        assert per.tolist() == [64, 17] and sorted(c.named) == sorted(tc.CORNER_KINDS)
        assert sorted(c.named.values()) == tc.CORNER_RANKS == [0, 15, 16, 63, 64, 80]
        assert (c.ip_id0 + c.named["ones"]) & 0xFFFF == 0xFFFF
        out, idx, count = c.want(c.n)
        assert count == 81
        lines = out.reshape(-1, 64)
        for kind, k in c.named.items():
            seen.add((kind, k))
            # the reset of that rank is the corner line's, for the id it carries
            line = tc.corner_offender(kind, (c.ip_id0 + k) & 0xFFFF)
            assert c.pool.reshape(-1, 64)[c.off[idx[k]]].tobytes() == line
            assert lines[k].tobytes() == ref.one(line, c.ip_id0 + k, tc.MAC)
            if kind in ("ip", "both"):
                assert not lines[k, 24:26].any()
            if kind in ("tcp", "both"):
                assert not lines[k, 50:52].any()
    assert seen == {(kind, k) for kind in tc.CORNER_KINDS for k in tc.CORNER_RANKS}
