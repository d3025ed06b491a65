"""CPU: the deterministic sets of tests/txplan_cases.py cover what they claim (no GPU: the sets and
the host planner only), and the constants they name are the kernel file's."""
import os
import re

import numpy as np
import pytest

import rxg
import txplan_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in tc.all_cases()}


def test_constants_are_the_kernel_files():
    src = open(os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc", "rxg_txplan.hip")).read()
    assert int(re.search(r"constexpr uint32_t kTile = (\d+);", src).group(1)) == tc.TILE
    assert int(re.search(r"constexpr uint32_t kScanLanes = (\d+);", src).group(1)) * tc.TILE == tc.SCAN_ROUND
    assert "wave * 64u + lane" in src and tc.SLICE == 64 and tc.SCAN_WAVE == 64 * tc.TILE


def test_send_counts_on_both_sides_of_every_edge(cases):
    have = {len(c["sends"]) for c in cases.values()}
    for edge in (tc.SLICE, tc.TILE, tc.SCAN_WAVE, tc.SCAN_ROUND):
        assert {edge - 1, edge, edge + 1} <= have, edge
    assert {1, 63, 2 * tc.TILE + 1} <= have
    for n in tc.ROUND_COUNTS:  # several segments at both ends and on the scan round's last tile
        ns = tc.nseg(cases[f"round_{n}"])
        assert ns[0] == 3 and ns[-1] == 3 and ns[tc.SCAN_ROUND - 2] == 3 and int(ns.min()) == 1
    for n in tc.SEND_COUNTS:
        if n >= 64:  # every block kind and refused sends among them
            c = cases[f"count_{n}"]
            assert set(range(8)) <= set(c["send_opt"].tolist()) and 0 < tc.refused(c).sum() < n


def test_byte_edges(cases):
    for k, m in ((tc.K_NONE, tc.MSS), (tc.K_O12, tc.MSS - 12)):
        c = cases[f"bytes_edges_block{k}"]
        assert (tc.cut(c) == m).all()
        assert {0, 1, m - 1, m, m + 1} <= set(c["sends"]["bytes"].tolist())
        assert tc.nseg(c).tolist() == [1, 1, 1, 1, 2, 2, 2, 3]


def test_lane_placement(cases):
    c = cases["lanes_63_64_65"]
    ns, first = tc.nseg(c).astype(np.int64), tc.first_of(c).astype(np.int64)
    for N in tc.LANE_NSEG:
        j = np.nonzero(ns == N)[0]
        assert {0, 63} <= set((first[j] % 64).tolist()), N
        assert {0, 63} <= set(((first[j] + N - 1) % 64).tolist()), N
    assert (c["sends"]["bytes"] % tc.LANE_MSS != 0).all()  # every last segment is a remainder


def test_big_sets(cases):
    assert tc.nseg(cases["big_alone"]).tolist() == [tc.BIG]
    assert tc.nseg(cases["big_between"]).tolist() == [1, 1, 1, tc.BIG, 1, 1]
    c = cases["one_segment_sends_2^16+1"]
    assert len(c["sends"]) == (1 << 16) + 1 and (tc.nseg(c) == 1).all()


def test_flags_wraps_offsets(cases):
    c = cases["flags_16x3"]
    ns, fl = tc.nseg(c), c["sends"]["tcp_flags"]
    mask = tc.SYN | tc.FIN | tc.PSH | tc.ACK
    for n in (1, 2, 3):
        assert sorted(set((fl[ns == n] & mask).tolist())) == sorted(
            {(tc.SYN * a) | (tc.FIN * b) | (tc.PSH * p) | (tc.ACK * k) for a in (0, 1) for b in (0, 1) for p in (0, 1)
             for k in (0, 1)})
        assert (ns == n).sum() == 16
    c = cases["wraps"]
    s, ns = c["sends"], tc.nseg(c)
    assert int(s["next_seq"][0]) == 0xFFFFFFFF and int(s["next_seq"][1]) == (1 << 32) - tc.MSS * tc.WRAP_NSEG + 1
    assert ns[0] == ns[1] == tc.WRAP_NSEG and int(s["ip_id0"][2]) == 0xFFFE and ns[2] == 5
    segs = rxg.tx_plan(s, tc.MSS)[0]
    assert segs["ip_id"][8:13].tolist() == [0xFFFE, 0xFFFF, 0, 1, 2]
    assert (segs["seq"][:8] < s["next_seq"][0]).any()  # the sequence numbers do wrap
    c = cases["src_off_2^40+7"]
    assert int(c["sends"]["src_off"][0]) == (1 << 40) + 7 and tc.nseg(c)[0] == 4

    def carries(c, j):
        """src_off's low word + q * m of send j's last segment reaches 2^32, that of segment 0 does not."""
        low = int(c["sends"]["src_off"][j]) & 0xFFFFFFFF
        return low < 1 << 32 <= low + (int(tc.nseg(c)[j]) - 1) * int(tc.cut(c)[j])
    assert carries(c, 1) and not carries(c, 0) and int(c["sends"]["src_off"][1]) == tc.CARRY_OFF
    # the planner's own descriptors of that send: the high word moves from 2^8 to 2^8 + 1
    assert (rxg.tx_plan(c["sends"], tc.MSS)[0]["src_off"][4:8] >> 32).tolist() == [256, 257, 257, 257]
    c = cases["bytes_2^32-1"]
    # 2^32 - 1 bytes at mss 65 481: 65 592 segments, the last one a remainder of 3 024 bytes; q * m
    # itself stays below 2^32 (it passes 2^31), and from segment 1 on src_off + q * m carries out of
    # src_off's low word (2^32 - 7) into its high word
    assert c["mss"] == 65481 and tc.nseg(c).tolist() == [1, 65592, 1]
    assert (1 << 32) - 1 - 65591 * 65481 == 3024 and 1 << 31 < 65591 * 65481 < 1 << 32
    assert int(c["sends"]["src_off"][1]) == tc.CARRY_OFF and carries(c, 1)
    assert (tc.CARRY_OFF & 0xFFFFFFFF) + 65481 >= 1 << 32


def test_blocks_and_refused(cases):
    c = cases["blocks_in_one_slice"]
    assert len(c["sends"]) == 64 and set(tc.cut(c).tolist()) == {tc.MSS, tc.MSS - 4, tc.MSS - 12, tc.MSS - 40}
    assert (c["send_opt"] == 0).any() and not tc.refused(c).any()
    kinds, shapes = set(), set()
    for name, c in cases.items():
        if not name.startswith("refused_"):
            continue
        r = tc.refused(c)
        assert r.any()
        kinds |= set(c["send_opt"][r].tolist())
        shapes |= {"first"} if r[0] else set()
        shapes |= {"last"} if r[-1] else set()
        shapes |= {"pair"} if (r[:-1] & r[1:]).any() else set()
    assert kinds >= {tc.K_PAST, tc.K_LEN44, tc.K_LEN6, tc.K_O40} and shapes == {"first", "last", "pair"}
    c = cases["refused_mss_eq_O"]
    assert c["mss"] == 40 and tc.refused(c).tolist() == [True, False, False, True, True, False, True]
    assert set((np.nonzero(tc.refused(cases["refused_lanes"]))[0] % 64).tolist()) == {0, 31, 32, 63}
    assert tc.refused(cases["refused_all"]).all() and tc.first_of(cases["refused_all"])[-1] == 0


def test_caps_and_nulls(cases):
    total = int(tc.first_of(cases["cap_total+0"])[-1])
    assert [tc.cap_of(cases[n]) for n in ("cap_total+0", "cap_total-1", "cap_0")] == [total, total - 1, 0]
    c = cases["cap_first+0"]
    f = tc.first_of(c)
    assert f[tc.CAP_SEND + 1] - f[tc.CAP_SEND] == 3 and 0 < f[tc.CAP_SEND] < f[-1]
    assert tc.cap_of(c) == f[tc.CAP_SEND] and tc.cap_of(cases["cap_first+1"]) == f[tc.CAP_SEND] + 1
    assert cases["send_opt_null"]["send_opt"] is None and cases["next_seq_null"]["next_seq"] is False
    assert len(cases["opts_null"]["opts"]) == 0


def test_expectations_come_from_the_host_planner(cases):
    """expect() on the small sets: all 32 bytes of every descriptor are the planner's, the
    refused sends are counted and keep their next_seq, the fill stands behind every end."""
    for name, c in cases.items():
        if tc.size_of(c) > tc.SMALL:
            continue
        w = tc.expect(c)
        n, nb = len(c["sends"]), min(w["total"], w["cap"])
        assert (w["segs"][nb * 32:] == tc.FILL).all() and len(w["segs"]) == (w["cap"] + tc.GUARD) * 32
        assert w["first"][n] == w["total"] and (np.diff(w["first"][:n + 1].astype(np.int64)) >= 0).all()
        assert (w["first"][n + 1:] == 0xA5A5A5A5A5A5A5A5).all() and (w["next_seq"][n:] == 0xA5A5A5A5).all()
        r = tc.refused(c)
        assert w["count"].tolist() == [w["total"], int(r.sum())]
        if c["next_seq"]:
            assert np.array_equal(w["next_seq"][:n][r], c["sends"]["next_seq"][r])
        else:
            assert (w["next_seq"] == 0xA5A5A5A5).all()
        if not r.any() and w["cap"] >= w["total"]:
            segs, nxt = rxg.tx_plan_opt(c["sends"], c["mss"], c["send_opt"], c["opts"])
            assert w["segs"][:nb * 32].tobytes() == segs.tobytes()
            assert rxg.tx_plan_count(c["sends"], c["mss"], c["send_opt"], c["opts"]) == w["total"]
