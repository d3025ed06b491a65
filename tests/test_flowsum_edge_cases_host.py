"""CPU: the edge sets of tests/flowsum_edge_cases.py held to their claims by the structural model
(which wave takes which slice on max_blocks 1, 2 and 3, which slices are wave-uniform, what each
wave carries, commits and ends on), every set through rxg_flow_sums_host against the numpy model
tests/flowsum_ref.py (so the GPU file's comparison is three-way), and the model against the
hand-written vectors of tests/golden/flowsum_kat.json that name their record kinds or frame
lengths."""
import numpy as np
import pytest

import flowsum_cases as cases
import flowsum_edge_cases as ec
import flowsum_ref as ref
import rxg
from test_flowsum_host import ALL_KATS, check, kat_records

TILE, ROUND = ec.TILE, ec.ROUND


def hold(c):
    """The case's claims on every max_blocks it names, REC8's fields kept by the 8-byte record,
    and the host function equal to the model in every kind; the model's answers per kind."""
    for mb in c.blocks:
        c.claim(c.structure(mb))
    got = {}
    for kind in c.kinds:
        if kind == rxg.REC8:
            back = rxg.rec8_expand(rxg.rec8_pack(np.ascontiguousarray(c.rec48["c"])))
            for f in ("tcb_idx", "verdict", "state", "tcp_flags", "flags", "datalen"):
                assert np.array_equal(back[f], c.rec48["c"][f]), (c.name, f, "does not fit an 8-byte record")
        got[kind] = check(c.rec48, kind, c.ntcb, c.frames(kind), c.flags, what=f"{c.name}, records of {kind}")
    return got


# ------------------------------------------------------------------ the model itself ---
def test_grid_by_hand():
    # 13 slices, max_blocks 3: ceil(13 / 4) = 4 > 3 workgroups, 12 waves, per = ceil(13 / 12) = 2
    assert ec.grid(13 * 64, 3) == (13, 3, 2, [(0, 2), (2, 4), (4, 6), (6, 8), (8, 10), (10, 12), (12, 13)] + [(13, 13)] * 5)
    # 5 slices, max_blocks 3: ceil(5 / 4) = 2 workgroups, 8 waves, per 1: three empty waves
    assert ec.grid(5 * 64 - 63, 3) == (5, 2, 1, [(k, k + 1) for k in range(5)] + [(5, 5)] * 3)
    assert ec.grid(1, 1) == (1, 1, 1, [(0, 1), (1, 1), (1, 1), (1, 1)])
    assert ec.grid(9 * 64, 1) == (9, 1, 3, [(0, 3), (3, 6), (6, 9), (9, 9)])


def test_structure_by_hand():
    # slices: 9 | 9 | nothing | 9 and 4 mixed | 2 | 2 ; max_blocks 1 -> per 2
    tcb = np.repeat([9, 9, 9, 9, 2, 2], 64)
    tcb[3 * 64 + 5] = 4
    r = cases.craft(tcb, datalen=7)
    c = r["c"]
    c["verdict"][128:192] = rxg.V_ARP
    r["c"] = c
    st = ec.Structure(r["c"], 16, 0, 1)
    assert (st.per, st.uniform) == (2, [9, 9, ec.NONE, ec.MIXED, 2, 2])
    assert st.carried == [[(9, [0, 1])], [], [(2, [4, 5])], []] and st.commits == [[], [], [], []]
    assert st.mixed == [[], [(3, ec.NONE, {9, 4})], [], []] and st.groups == [[9, ec.NONE, 2, ec.NONE]]
    assert st.lane_bytes([0, 1]).tolist() == [14] * 64
    st = ec.Structure(r["c"], 16, 0, 3)            # 6 slices: 2 workgroups, per 1
    assert st.groups == [[9, 9, ec.NONE, ec.NONE], [2, 2, ec.NONE, ec.NONE]]
    st = ec.Structure(r["c"][:5 * 64], 16, 0, 1)   # per 2: wave 1 is [nothing, mixed], wave 2 ends on 2
    st4 = ec.Structure(r["c"], 4, 0, 1)            # ntcb 4: flows 9 and 4 are out of range
    assert st.groups == [[9, ec.NONE, 2, ec.NONE]] and st4.uniform == [ec.NONE] * 4 + [2, 2] and int(st4.out.sum()) == 192


def test_rec8_datalen_range_round_trips():
    assert ec.REC8_MAX_DATALEN == 130943
    r = cases.craft([0, 0, 0, 0], datalen=[ec.REC8_MIN_DATALEN, ec.REC8_MAX_DATALEN, ec.REC8_MAX_DATALEN + 1, -129])["c"]
    back = rxg.rec8_expand(rxg.rec8_pack(np.ascontiguousarray(r)))["datalen"].tolist()
    assert back == [ec.REC8_MIN_DATALEN, ec.REC8_MAX_DATALEN, -128, ec.REC8_MAX_DATALEN]      # the field holds 17 bits


# --------------------------------------------------------------------------- the sets ---
@pytest.mark.parametrize("mb", ec.BLOCKS)
@pytest.mark.parametrize("place", ec.PLACES)
def test_meet(place, mb):
    cs = ec.meet_cases(place, mb)
    assert len(cs) == (0 if (place[0] == "d" and mb == 1) else 17)
    for c in cs:
        want = hold(c)[c.kinds[0]][0]
        f = want[np.searchsorted(want["tcb_idx"], ec.F)]
        v = ec.variants(c.kinds[0])[c.name.split(", ")[1]]
        assert int(f["tcb_idx"]) == ec.F and int(f["frames"]) == len(v) and int(f["state"]) == v[0]["state"] != v[-1]["state"]
        assert int(f["max_seq"]) == max(x["seq"] for x in v) and int(f["max_ack"]) == max(x["ack"] for x in v)
        assert int(f["tcp_flags_or"]) == int(np.bitwise_or.reduce([x["tcp_flags"] for x in v]))
        assert int(f["data_bytes"]) == sum(x["datalen"] for x in v if x["datalen"] > 0)
        assert int(f["first_idx"]) < int(f["last_idx"])


def test_meet_c_on_one_workgroup_by_name():
    c = ec.meet_case("c lds merge", "hi", rxg.REC16, 1)
    st = c.structure(1)
    assert st.runs == [(0, 3), (3, 6), (6, 9), (9, 12)] and st.ends[1] == st.ends[2] == ec.F
    assert st.groups == [[102, ec.F, ec.F, 111]]
    c = ec.meet_case("b register carry", "bytes", rxg.REC48, 2)
    st = c.structure(2)
    assert st.carried[1] == [(ec.F, [3, 4, 5])] and int(st.lane_bytes([3, 4, 5])[17]) == 3 * ec.INT32_MAX > 2**32
    assert int(st.lane_bytes([3, 4])[17]) < 2**32 and (np.delete(st.lane_bytes([3, 4, 5]), 17) == 0).all()


@pytest.mark.parametrize("pattern", ec.LDS_PATTERNS)
def test_lds(pattern):
    for kind in ec.KINDS:
        c = ec.lds_case(pattern, kind)
        assert c.structure(1).groups == [[{"A": 31, "B": 32, "C": 2047, "D": 2048, ".": ec.NONE}[ch] for ch in pattern]]
        want = hold(c)[kind][0]
        assert len(want) == len(set(pattern) - {"."})
        if kind != rxg.REC8:
            assert (want["data_bytes"] > 2**36).all()


@pytest.mark.parametrize("mb", ec.BLOCKS)
def test_runs(mb):
    cs = ec.run_cases(mb)
    assert len(cs) == 3 * 7 * 2 and {k for c in cs for k in c.kinds} == set(ec.KINDS)
    for c in cs:
        hold(c)
    nw = 4 * mb
    one = {c.n: c.structure(mb) for c in cs if c.name.startswith("runs one flow")}
    assert one[64 * (nw - 1)].empty_waves() == [nw - 1] and one[64 * nw].empty_waves() == []
    assert one[64 * (nw + 1)].per == 2 and len(one[64 * (nw + 1)].empty_waves()) == nw - (nw + 2) // 2
    assert one[64 * (3 * nw + 1)].per == 4 and one[64 * (3 * nw + 1) - 63].runs[(3 * nw) // 4] == (3 * nw, 3 * nw + 1)
    two = next(c for c in cs if c.name.startswith("runs a flow per two slices") and c.n == 64 * (2 * nw + 1))
    st = two.structure(mb)             # per 3 cuts the trains of two: a wave carries a whole one and half of the next
    assert st.per == 3 and st.carried[0] == [(10, [0, 1]), (11, [2])] and st.carried[1] == [(11, [3]), (12, [4, 5])]


def test_left():
    cs = ec.left_cases()
    for c in cs:
        got = hold(c)
        counts = {tuple(w[1].tolist()) for w in got.values()}
        assert len(counts) == 1
    by = {c.name: c for c in cs}
    st = by["left both kinds mixed with counted frames"].structure(2)
    assert st.ablocks == 2 and min(min(st.left_of_wave(w)) for w in range(8)) > 20
    assert int(st.out.sum()) > 300 and int(st.nok.sum()) > 300
    big = by["left whole slices out of range, nothing counted"]
    assert set(ec.bad_tcbs(big.ntcb)) == set(big.rec48["c"]["tcb_idx"].tolist())
    assert set(by["left the 255 other verdicts are ignored"].rec48["c"]["verdict"].tolist()) == set(range(256))
    assert set(by["left the 7 other verdicts are ignored"].rec48["c"]["verdict"].tolist()) == set(range(8))


@pytest.mark.parametrize("kind", ec.KINDS)
def test_decode(kind):
    c = ec.decode_case(kind)
    want = hold(c)[kind][0]
    assert set(want["tcp_flags_or"].tolist()) >= {1, 2, 4, 8, 16, 32, 64, 128, 255, 0}
    states = set(range(7)) | {rxg.STATE_NONE} | ({8, 10, 0xFE} if kind != rxg.REC8 else set())
    assert set(want["state"].tolist()) == states and len(want) == c.ntcb
    top = ec.REC8_MAX_DATALEN if kind == rxg.REC8 else ec.INT32_MAX
    assert int(want["data_bytes"].max()) == top and int((want["frames"] == 2).sum()) == 2 * len(states) - 2
    pairs = want[want["frames"] == 2]
    assert (c.rec48["c"]["state"][pairs["first_idx"]] == pairs["state"]).all()
    assert (c.rec48["c"]["state"][pairs["last_idx"]] != pairs["state"]).all()


def test_frames():
    names = [name for name, _, _ in ec.frame_forms()]
    assert len(names) == 6 and {int(n.split()[1]) for n in names if n.startswith("stride")} == {1, 2, 1024}
    for name, c, build in ec.frame_forms():
        frames = c.frames(rxg.REC16)
        k = c.n // 2
        assert [len(f) for f in frames[:k]] == [ln for ln in ec.FRAME_LENS if ln <= max(len(f) for f in frames)]
        pool, off, lens, geom = build(frames)
        for f, o, ln in zip(frames, off.tolist(), lens.tolist()):          # the pool: each frame, then 0xFF up to the next slot
            assert pool[o * 64:o * 64 + ln].tobytes() == f and ln == len(f)
            assert (pool[o * 64 + ln:(o + max(1, (ln + 63) // 64)) * 64] == 0xFF).all()
        assert geom is None or off.tolist() == [geom[0] + i * geom[1] for i in range(c.n)]
        if "shuffled" in name:
            assert sorted(off.tolist()) != off.tolist() and len(set(off.tolist())) == c.n
    c = ec.frames_case()
    want = hold(c)[rxg.REC8][0]
    by_len = dict(zip(ec.FRAME_LENS, zip(want["max_seq"].tolist(), want["max_ack"].tolist())))
    assert by_len[0] == by_len[37] == by_len[38] == (0x102, 1)               # the second frame's
    assert by_len[39] == (0xA1000000, 1) and by_len[41] == (0xA1B2C300, 1) and by_len[42] == (0xA1B2C3D4, 1)
    assert by_len[43] == (0xA1B2C3D4, 0xE5000000) and by_len[45] == (0xA1B2C3D4, 0xE5F60700)
    for ln in (46, 47, 64, 65, 0x7FFF, 0x8000, 0xFFFF):
        assert by_len[ln] == (0xA1B2C3D4, 0xE5F60718), ln


@pytest.mark.parametrize("kind", ec.KINDS)
def test_cap(kind):
    c = ec.cap_case(kind)
    want = hold(c)[kind][0]
    m = len(want)
    assert m == 150 and want["tcb_idx"][[31, 32, 63, 64]].tolist() == [31, 32, TILE - 1, TILE]
    for cap in ec.caps(m):
        if cap <= m + 1:                     # the host function gets a buffer of cap + guard entries
            check(c.rec48, kind, c.ntcb, c.frames(kind), cap=cap, what=f"cap {cap}")
    assert sorted(ec.caps(m)) == ec.caps(m) and {m - 1, m, m + 1, 2**32, 2**64 - 1} <= set(ec.caps(m))


@pytest.mark.parametrize("ntcb", ec.SCAN_NTCB)
def test_scan(ntcb):
    c = ec.scan_case(ntcb)
    flows = c.flows
    ntiles = (ntcb + TILE - 1) // TILE
    assert ntiles == {ec.SCAN_NTCB[0]: ROUND - 1, ec.SCAN_NTCB[1]: ROUND, ec.SCAN_NTCB[2]: ROUND, ec.SCAN_NTCB[3]: ROUND + 1,
                      ec.SCAN_NTCB[4]: 8 * ROUND}[ntcb]
    per_tile = np.bincount(flows // TILE, minlength=ntiles)
    full = [t for t in (ROUND - 1, ROUND) if t < ntiles]         # every entry the table has in them: 2 047, 2 048 or 1
    assert all(per_tile[t] == min(TILE, ntcb - t * TILE) for t in full) and len(full) == min(2, max(0, ntiles - ROUND + 1))
    edge = {t for e in range(ROUND, ntiles + 1, ROUND) for t in (e - 1, e) if t < ntiles}
    for t in edge:
        assert t * TILE in flows and (t * TILE + TILE - 1 in flows or t * TILE + TILE - 1 >= ntcb), t
    plain = [t for t in range(ntiles) if t not in edge and t not in full]
    assert all(per_tile[t] == t % 5 for t in plain) and len(plain) >= ntiles - 16
    if ntcb == ROUND * TILE + 1:
        assert flows[-1] == ROUND * TILE            # the one flow of the one-entry last tile
    want = hold(c)[rxg.REC16][0]
    assert want["tcb_idx"].tolist() == flows.tolist() and c.n < 30000


# ---------------------------------------------------------------- hand-written vectors ---
EDGE_KATS = ALL_KATS[3:]


def test_the_vectors_are_the_four_asked_for():
    names = " | ".join(k["name"] for k in EDGE_KATS)
    assert len(EDGE_KATS) == 4 and all(w in names for w in ("first frame's", "one tcp_flags bit", "passes 2^32", "0x8000"))


@pytest.mark.parametrize("k", EDGE_KATS, ids=[k["name"][:40] for k in EDGE_KATS])
def test_known_answers(k):
    r = kat_records(k)
    frames = ec.frames_of(r, k["lens"], fill=0xFF) if "lens" in k else None
    for kind in k.get("kinds", ec.KINDS):
        want, count = check(r, kind, k["ntcb"], frames, flags=k["flags"], what=k["name"])
        assert [list(ref.as_tuple(w)) for w in want] == k["want"]          # the model gives the hand-written answers
        assert count.tolist() == k["count"]
