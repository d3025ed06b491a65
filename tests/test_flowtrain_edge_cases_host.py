"""CPU: the edge sets of tests/flowtrain_edge_cases.py held to their claims (which slice carries a
left-out count, which wave-round of which tile holds a digit before each pass, which sorted
position starts a train), every set through rxg_flow_trains_host against the numpy model
tests/flowtrain_ref.py in every layout (so the GPU file's comparison is three-way), the small sets
through the stand-alone program tests/flowtrain_check.cpp plain and under ASan/UBSan, and a
statement that the sets of tests/flowtrain_cases.py do not reach these places."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import flowtrain_cases as cases
import flowtrain_edge_cases as ec
import flowtrain_ref as ref
import rxg
from test_flowtrain_host import FILL, INC, ROOT, compare, expect, host_raw

EDGE = ec.edge_cases()
TILE, ROUND, WAVE = ec.TILE, ec.ROUND, ec.WAVE
KEYS = {"n", "slices", "out", "left", "out_at", "left_at", "passes", "tiles", "S", "T", "digits", "multi", "odd", "firsts",
        "hole", "long", "cap_trains", "heads", "head_flow", "counts", "kinds"}


def model(case):
    return ref.trains(case.rec48, rxg.REC48, case.ntcb, None, case.flags, case.cur_array())


# ------------------------------------------------------------ the constants and helpers ---
def test_constants_and_helpers_by_hand():
    kh = open(os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc", "rxg_kernels.h")).read()
    assert int(re.search(r"kFtScanPer = (\d+)", kh).group(1)) == ec.SCAN_PER
    assert int(re.search(r"kFtScanLanes = (\d+)", kh).group(1)) == ec.SCAN_LANES
    assert ec.SUBS * WAVE == TILE and TILE % ROUND == 0 and ROUND % WAVE == 0
    assert ec.TOP_NTCB - 1 >= 1 << 16 and ec.TOP_NTCB - 1 <= ec.fc.REC8_MAX_TCB
    assert ec.LARGEST == max(c.n for c in EDGE) and ec.LARGEST * 64 < 5 << 20
    assert ec.per_slice(np.arange(130) % 2 == 0).tolist() == [32, 32, 1]
    # 0x0201 0x0102 0x0001: pass 0 reads packet order, pass 1 the order of the low digit (stable)
    p = ec.pass_inputs([0x0201, 0x0102, 0x0001], 2)
    assert p[0].tolist() == [0x0201, 0x0102, 0x0001] and p[1].tolist() == [0x0201, 0x0001, 0x0102]
    a, b = ec.craft([1, 1], [5, 6], 1), ec.craft([2, 2, 2], [7, 8, 9], 1)
    m = ec.interleave([a, b], seed=1)
    assert m["seq"][m["c"]["tcb_idx"] == 1].tolist() == [5, 6] and m["seq"][m["c"]["tcb_idx"] == 2].tolist() == [7, 8, 9]
    seg, out, left = ec.kinds_of(ec.decode_cases()[0].rec48, 3, rxg.FT_TCP_OK_ONLY)
    assert (seg.tolist(), out.tolist(), left.tolist()) == ([True] * 2 + [False] * 5, [False, False, True, True, False, False, True],
                                                           [False] * 4 + [True] + [False] * 2)


# ------------------------------------------------------------------------- the claims ---
def test_every_claim_an_edge_set_makes_holds_in_the_model():
    assert len({c.name for c in EDGE}) == len(EDGE) and not {c.name for c in EDGE} & {c.name for c in cases.rule_cases()}
    seen = set()
    for case in EDGE:
        order, trains, count = model(case)
        cl, name = case.claims, case.name
        assert set(cl) <= KEYS, name
        seen |= set(cl)
        S, T = int(count[0]), int(count[1])
        seg, out, left = ec.kinds_of(case.rec48, case.ntcb, case.flags)
        assert int(seg.sum()) == S and int(trains["nseg"].sum()) == S, name
        keys = case.rec48["c"]["tcb_idx"][seg].astype(np.int64)            # the sort's input: the segments in packet order
        if "n" in cl:
            assert case.n == cl["n"] and len(ec.per_slice(seg)) == cl["slices"], name
        if "out" in cl:
            assert (int(count[2]), int(count[3])) == (cl["out"], cl["left"]) == (int(out.sum()), int(left.sum())), name
            po, pl = ec.per_slice(out), ec.per_slice(left)
            assert {s: int(k) for s, k in enumerate(po) if k} == cl["out_at"], name
            assert {s: int(k) for s, k in enumerate(pl) if k} == cl["left_at"], name
            assert case.flags == rxg.FT_TCP_OK_ONLY and S > 0, name
        if "S" in cl:
            assert S == cl["S"], (name, S)
        if "T" in cl:
            assert T == cl["T"], (name, T)
        if "tiles" in cl:
            assert -(-S // TILE) == cl["tiles"], name
        if "passes" in cl:
            top = int(keys.max())
            need = 1 if top < 1 << 8 else 2 if top < 1 << 16 else 3
            assert cl["passes"] == cases.passes_needed(case.ntcb) == need and top < case.ntcb, name
        if "digits" in cl:
            for p, inp in enumerate(ec.pass_inputs(keys, cl["passes"])):
                digits = set(((inp >> (8 * p)) & 0xFF).tolist())
                assert len(digits) >= cl["digits"] and {0x00, 0xFF} <= digits, (name, p)
                for t, tile in enumerate(ec.tiles_of(inp)):                  # the last tile holds five pairs
                    assert len(set(((tile >> (8 * p)) & 0xFF).tolist())) >= 2, (name, p, t)
            assert int((trains["nseg"] > 1).sum()) >= cl["multi"], name
            same = np.nonzero(np.diff(np.sort(keys, kind="stable")) == 0)[0]
            assert len(same) > S // 2, name                                  # equal keys: their packet order must survive
        if "odd" in cl:
            tile, sub = cl["odd"]
            inp = ec.pass_inputs(keys, 1)[0]
            at = np.nonzero((inp & 0xFF) == 0xFF)[0]
            assert len(at) == 1 and (int(at[0]) // TILE, int(at[0]) % TILE // WAVE) == (tile, sub), name
            assert set(inp.tolist()) == {0, 0xFF}, name
        if "firsts" in cl:
            assert trains["first"].tolist() == cl["firsts"] and int(seg.sum()) == case.n, name
        if "hole" in cl:
            t = cl["hole"]
            assert not ((trains["first"] >= t * TILE) & (trains["first"] < (t + 1) * TILE)).any(), name
            assert ((trains["first"] < t * TILE).any() and (trains["first"] >= (t + 1) * TILE).any()), name
            first, nseg, nbytes = cl["long"]
            tr = trains[trains["tcb_idx"] == 1]
            assert len(tr) == 1 and (int(tr[0]["first"]), int(tr[0]["nseg"]), int(tr[0]["bytes"])) == (first, nseg, nbytes), name
            dl = case.rec48["c"]["datalen"][case.rec48["c"]["tcb_idx"] == 1]
            assert nbytes == int(dl.astype(np.int64).sum()) and nseg == 2 * TILE + 7, name
            assert cl["cap_trains"] == [T, T - 1, 5], name
        if "heads" in cl:
            heads = trains[(trains["flags"] & rxg.FTR_HEAD) != 0]
            assert len(heads) == cl["heads"] == 1 and int(heads[0]["tcb_idx"]) == cl["head_flow"] == case.ntcb - 1, name
            cur, top = case.cur_array(), case.ntcb - 1
            assert int(cur[top]) == int(heads[0]["seq"]), name
            for cut in (top & 0xFFFF, top & 0xFF):                          # the index cut short names another entry,
                if cut != top:                                              # which holds no seq that would make a HEAD
                    mine = trains[trains["tcb_idx"] == cut]
                    assert len(mine) == 1 and int(cur[cut]) not in (0, int(heads[0]["seq"]), int(mine[0]["seq"])), name
                    assert int(cur[cut]) in trains["seq"].tolist(), name
            assert any(cut != top for cut in (top & 0xFFFF, top & 0xFF)), name
        if "counts" in cl:
            assert count.tolist() == cl["counts"], (name, count)
            for kind in ec.kinds(case):                                      # the same in every layout the set runs in
                recs, frames, want = expect(case, kind)
                assert want[2].tolist() == cl["counts"], (name, kind)
    assert seen == KEYS
    by = {c.name: c for c in EDGE}
    # the sets the issue names by size and place
    a, b, c = ec.counter_cases()[:3]
    assert (a.claims["slices"], a.n) == (WAVE + 1, WAVE * WAVE + 17) and set(a.claims["out_at"]) == set(a.claims["left_at"]) == {WAVE}
    assert a.claims["out"] != a.claims["left"]
    assert (b.claims["slices"], b.n) == (ec.SCAN_LANES + 1, ec.SCAN_LANES * WAVE + 3) and set(b.claims["out_at"]) == {ec.SCAN_LANES}
    assert b.claims["out"] != b.claims["left"] and set(b.claims["left_at"]) == {ec.SCAN_LANES}
    assert c.n == b.n and set(c.claims["out_at"]) | set(c.claims["left_at"]) == set(range(ec.SCAN_LANES + 1))
    assert c.claims["out_at"][5] == WAVE and c.claims["left_at"][70] == WAVE
    assert all(min(c.claims["out_at"].get(s, 0), c.claims["left_at"].get(s, 0)) >= 1 for s in range(ec.SCAN_LANES + 1) if s not in (5, 70))
    d, e = ec.counter_cases()[3:]
    assert (d.claims["out"], d.claims["left"], e.claims["out"], e.claims["left"]) == (1, 0, 0, 1)
    assert list(d.claims["out_at"]) == list(e.claims["left_at"]) == [d.claims["slices"] - 1]
    assert ec.EDGES == [63, 64, 255, 256, 1023, 1024, 2048] and ec.AFTER == [65, 257, 1025, 2049]
    assert sorted({p // WAVE for p in ec.digit_positions()}) == [0, 1, 14, ec.SUBS - 1] and len(ec.digit_cases()) == 8
    assert [c.claims["T"] for c in ec.emit_cases()[:4]] == [255, 256, 257, 256]
    assert [c.ntcb for c in ec.emit_cases()[4:]] == [257, 65537, ec.TOP_NTCB] and ec.pass_cases()[0].ntcb == ec.TOP_NTCB
    assert ec.kinds(by["decode: tcb_idx INT32_MIN and INT32_MAX"]) == ec.BIG
    idx = by["decode: tcb_idx INT32_MIN and INT32_MAX"].rec48["c"]["tcb_idx"].tolist()
    assert ec.INT32_MIN in idx and ec.INT32_MAX in idx


# ------------------------------------------------------ the host function and the model ---
@pytest.mark.parametrize("case", EDGE, ids=lambda c: c.name)
def test_host_function_equals_the_model_on_every_edge_set(case):
    for kind in ec.kinds(case):
        recs, frames, want = expect(case, kind)
        S, T = int(want[2][0]), int(want[2][1])
        cur = case.cur_array()
        for cap_seg, cap_trains in [(S, T), (S - 1, T), (S, T - 1)] + [(S, t) for t in case.claims.get("cap_trains", [])]:
            got = host_raw(recs, kind, case.ntcb, frames, case.flags, cur, cap_seg, cap_trains)
            compare(got, want, cap_seg, cap_trains, f"{case.name}, records of {kind}, caps {cap_seg} {cap_trains}")


# ------------------------------------------- the host function stand-alone, sanitized too ---
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_function_standalone_on_the_small_edge_sets(tmp_path, san):
    """Built and driven as test_flowtrain_host.test_host_function_standalone does."""
    small = [c for c in EDGE if c.ntcb <= 70000 and c.n <= 2 * TILE + 64]
    # (the counter and pass sets are larger than that, the widest HEAD set's table is)
    assert {c.name.split(":")[0] for c in small} == {"digit", "starts", "hole", "emit", "decode"} and len(small) >= 29
    exe = tmp_path / "flowtrain_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *san, "-I", INC,
                    os.path.join(ROOT, "tests", "flowtrain_check.cpp"),
                    os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc", "rxg_flowtrain.cpp"), "-o", str(exe)], check=True)
    jobs = []
    blob = bytearray()
    for k, case in enumerate(small):
        ks = ec.kinds(case)
        kind = ks[k % len(ks)]
        recs, frames, want = expect(case, kind)
        S, T = int(want[2][0]), int(want[2][1])
        for cap_seg, cap_trains in ((S, T), (S - 1, T - 1)):
            cur = case.cur_array()
            blob += struct.pack("<7I", kind, case.n, case.ntcb, case.flags, cur is not None, cap_seg, cap_trains)
            blob += recs.tobytes()
            if frames is not None:
                for f in frames:
                    blob += struct.pack("<H", len(f)) + f
            if cur is not None:
                blob += cur.tobytes()
            jobs.append((case.name, want, cap_seg, cap_trains))
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", len(jobs)) + bytes(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0 and "flowtrain ok" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr
    out = (tmp_path / "out.bin").read_bytes()
    at = 0
    for name, want, cap_seg, cap_trains in jobs:
        rc, = struct.unpack_from("<i", out, at)
        count = np.frombuffer(out, np.uint64, 4, at + 4)
        order = np.frombuffer(out, np.uint32, cap_seg, at + 36)
        trains = np.frombuffer(out, rxg.FLOW_TRAIN_DTYPE, cap_trains, at + 36 + 4 * cap_seg)
        at += 36 + 4 * cap_seg + 32 * cap_trains
        s, t = min(len(want[0]), cap_seg), min(len(want[1]), cap_trains)
        assert rc == 0 and count.tolist() == want[2].tolist(), name
        assert order[:s].tolist() == want[0][:s].tolist() and (order[s:] == 0xA5A5A5A5).all(), name
        assert trains[:t].tobytes() == want[1][:t].tobytes() and (trains[t:].view(np.uint8) == FILL).all(), name
    assert at == len(out)


# ------------------------------------------- what the sets of flowtrain_cases.py reach ---
def test_the_rule_sets_do_not_reach_these_places():
    """No slice of index 64 or higher of any earlier set carries a left-out count (so only the
    first wave's lanes ever summed one, in the loop's first trip), and no earlier set that takes
    three passes holds more than one tile of segments.  SCAN_SIZES are the frame counts of
    test_gpu_flowtrain.test_scan_round_edges_on_three_grids, all segments of flows below 1 000."""
    for case in cases.rule_cases():
        seg, out, left = ec.kinds_of(case.rec48, case.ntcb, case.flags)
        assert not ec.per_slice(out)[WAVE:].any() and not ec.per_slice(left)[WAVE:].any(), case.name
        if cases.passes_needed(case.ntcb) >= 3:
            assert int(seg.sum()) <= TILE, case.name
    for n in cases.SCAN_SIZES:
        c = cases.big(n, seed=n)["c"]
        assert (c["verdict"] == rxg.V_DISPATCH).all() and int(c["tcb_idx"].min()) >= 0 and int(c["tcb_idx"].max()) < 1000
        assert (c["flags"] & rxg.F_TCP_OK).all() and cases.passes_needed(1000) == 2
    # and the new sets do: a count in slice 64, in slice SCAN_LANES, three passes over four tiles
    assert any(set(c.claims.get("out_at", {})) == {WAVE} for c in EDGE)
    assert any(set(c.claims.get("left_at", {})) == {ec.SCAN_LANES} for c in EDGE)
    assert any(c.claims.get("passes") == 3 and c.claims.get("tiles", 0) > 1 for c in EDGE)
