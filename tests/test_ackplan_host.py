"""CPU: rxg_ack_plan_host (a burst's ACKs planned per flow, host form) against the model
tests/ackplan_ref.py on every set of tests/ackplan_cases.py with whole-buffer compares, its -EINVAL
list, the model against the reference's receive window, the ACK frame against what
sendtcpdata(ptcb, NULL, 0) writes, and the host form stand-alone under ASan/UBSan.  The
rxg_acks_attach / rxg_ack_take rules need a context and a replay: tests/test_gpu_ackplan.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import ackplan_cases as cases
import ackplan_ref as ref
import flowtrain_cases as ftc
import oracle
import pktgen
import rxg
import trainpay_cases as tpc
import txbuild_opt_ref as oref
import txbuild_ref
from oracle import window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc")
EINVAL = 22
SETS = cases.all_sets()
NEW = ["rxg_ack_plan_dev", "rxg_ack_plan_host", "rxg_acks_attach", "rxg_ack_take"]


def plan_args(s, sg, ak, op, cnt, **over):
    a = s.args
    order, trains = s.order[:a["cap_seg"]], s.trains[:a["cap_trains"]]
    keep = [np.ascontiguousarray(order), np.ascontiguousarray(trains), s.train_count, s.state, s.rxopts]
    d = dict(order=keep[0].ctypes.data if len(order) else None, cap_seg=a["cap_seg"],
             trains=keep[1].ctypes.data if len(trains) else None, cap_trains=a["cap_trains"],
             train_count=s.train_count.ctypes.data, n=s.n, ntcb=s.ntcb,
             rxopts=s.rxopts.ctypes.data if s.rxopts is not None and len(s.rxopts) else None, state=s.state.ctypes.data,
             flags=0, tsval_now=a["tsval_now"], ip_id0=a["ip_id0"], pad0=0, opt_plain=a["opt_plain"],
             opt_base=a["opt_base"], opt_cap=a["opt_cap"], opts=op.ctypes.data if op is not None else None,
             segs=sg.ctypes.data, acks=ak.ctypes.data, cap=a["cap"], count=cnt.ctypes.data)
    d.update(over)
    return rxg.DevAckPlan(**d), keep


def run_host(s):
    (wsegs, wacks, wopts, wcount), _ = cases.expect(s)
    segs, acks = np.full_like(wsegs, 0), np.full_like(wacks, 0)
    segs.view(np.uint8)[:] = cases.FILL
    acks.view(np.uint8)[:] = cases.FILL
    opts = s.opts_in() if s.use_opts else None
    count = np.full(6, 0xA5A5A5A5A5A5A5A5, np.uint64)
    b, keep = plan_args(s, segs, acks, opts, count[1:])
    assert rxg.load_library().rxg_ack_plan_host(C.byref(b)) == 0
    assert count[[0, 5]].tolist() == [0xA5A5A5A5A5A5A5A5] * 2 and count[1:5].tolist() == wcount.tolist(), (s.name, count, wcount)
    assert segs.tobytes() == wsegs.tobytes(), (s.name, "segs", np.nonzero(segs != wsegs)[0][:5])
    assert acks.tobytes() == wacks.tobytes(), (s.name, "acks", np.nonzero(acks != wacks)[0][:5])
    if opts is not None:
        assert opts.tobytes() == wopts.tobytes(), (s.name, "opts", np.nonzero(opts != wopts)[0][:5])


# ------------------------------------------------- 1. the host form equals the model ---
@pytest.mark.parametrize("s", SETS, ids=[s.name for s in SETS])
def test_host_function_equals_the_model(s):
    run_host(s)


def test_every_claim_a_set_makes_holds_in_the_model():
    assert len({s.name for s in SETS}) == len(SETS)
    assert (cases.TILE, cases.SCAN, cases.ROUND) == (256, 256, 65536)
    by = {s.name: s for s in SETS}
    big = by[f"T={cases.ROUND + 1} mixed"]
    tcb = big.trains["tcb_idx"]
    firsts = np.nonzero(np.r_[True, tcb[1:] != tcb[:-1]])[0]
    lens = np.diff(np.r_[firsts, len(tcb)])
    assert set((firsts % 256).tolist()) == set(range(256)) and set(lens.tolist()) >= {1, 2, 3, 4, 5}
    assert (lens[firsts % 256 == 255] >= 2).all() and (firsts % 256 == 255).sum() > 10    # flows that straddle a tile edge
    assert (firsts % 256 == 0).sum() > 10
    segs, acks, count, blocks = big.model()
    assert count[0] > 256 * 40 and count[1] > 100 and len(blocks) > 100
    assert int(segs["ip_id"][16]) == 0 and int(segs["ip_id"][15]) == 0xFFFF                   # the wrap
    fl = acks["flags_train"] & 0xFF
    assert {rxg.ACK_ADVANCES, rxg.ACK_DUP, rxg.ACK_ADVANCES | rxg.ACK_FIN} <= set(fl.tolist())
    assert int(acks["flags_train"][-1] >> 8) >= cases.ROUND - 5                                 # a train past the scan's first round
    # the combinations: 8 LIVE flows, and the echo follows rxopts
    for name, echo in (("combos rxopts NULL", False), ("combos rxopts TS", True), ("combos rxopts no TS", False)):
        s = by[name]
        segs, acks, count, blocks = s.model()
        assert count.tolist() == [8, 8, 0, 0] and len(blocks) == 4
        for k, b in blocks.items():
            a = acks[k]
            f = int(a["tcb_idx"])
            tsecr = int.from_bytes(bytes(b["bytes"][8:12]), "big")
            adv = bool(int(a["flags_train"]) & rxg.ACK_ADVANCES)
            assert adv == bool(f & 2)
            want = 5000 + int(s.order[2 * f]) if (echo and adv) else int(s.state[f]["ts_recent"])
            assert tsecr == want, (name, f)
    assert by["combos opts NULL"].model()[2].tolist() == [8, 8, 0, 0] and not by["combos opts NULL"].model()[3]
    segs, acks, count, _ = by["tcb_idx -1, ntcb - 1, ntcb, 0x7FFFFFFF"].model()
    assert count.tolist() == [3, 0, 4, 0] and acks["tcb_idx"].tolist() == [0, 3, 8]
    assert by["ip_id0 0xFFF0 over 40 ACKs opt_cap 2"].model()[2].tolist() == [40, 0, 0, 20]
    assert by["ip_id0 0xFFF0 over 40 ACKs opt_cap 3"].model()[2].tolist() == [40, 0, 0, 19]
    assert by["ip_id0 0xFFF0 over 40 ACKs opt_cap 40"].model()[2].tolist() == [40, 0, 0, 1]
    assert by["ip_id0 0xFFF0 over 40 ACKs opt_cap 41"].model()[2].tolist() == [40, 0, 0, 0]
    s = by["ip_id0 0xFFF0 over 40 ACKs opt_cap 40"]
    assert int(s.model()[1]["flags_train"][38]) & rxg.ACK_NO_OPT and int(s.model()[0]["reserved"][38]) == 1
    assert by["ip_id0 0xFFF0 over 40 ACKs cap 0"].model()[2].tolist() == [40, 0, 0, 0]
    segs, acks, count, _ = by["FLOW_FIRST on a later train, missing on the first"].model()
    assert count[0] == 3 and (acks["flags_train"] >> 8).tolist() == [0, 3, 4]
    segs, acks, count, blocks = by["order[first] >= n"].model()
    s = by["order[first] >= n"]
    got = [int.from_bytes(bytes(blocks[k]["bytes"][8:12]), "big") for k in range(5)]
    rec = [int(s.state[k]["ts_recent"]) for k in range(5)]
    assert got == [5002, rec[1], rec[2], 5001, rec[4]]
    for name in ("T' 0: count[1] 0", "T' 0: count[0] 0", "T' 0: cap_trains 0", "n 0"):
        segs, acks, count, blocks = by[f"T=300 mixed {name}"].model()
        assert count.tolist() == [0, 0, 0, 0] and not len(segs) and not blocks


def test_errors_write_nothing():
    lib = rxg.load_library()
    s = cases.wrap_set()
    (wsegs, wacks, wopts, _), _ = cases.expect(s)
    bad = [dict(train_count=None), dict(state=None), dict(count=None), dict(order=None), dict(trains=None),
           dict(segs=None), dict(acks=None), dict(opt_plain=3), dict(opt_base=99), dict(ntcb=0),
           dict(ntcb=rxg.FS_MAX_NTCB + 1), dict(flags=1), dict(flags=0x80000000)]
    for over in bad:
        segs, acks = wsegs.copy(), wacks.copy()
        segs.view(np.uint8)[:] = cases.FILL
        acks.view(np.uint8)[:] = cases.FILL
        opts = s.opts_in()
        keep_opts = opts.copy()
        count = np.full(4, 0xA5A5A5A5A5A5A5A5, np.uint64)
        b, keep = plan_args(s, segs, acks, opts, count, **over)
        assert lib.rxg_ack_plan_host(C.byref(b)) == -EINVAL, over
        assert (segs.view(np.uint8) == cases.FILL).all() and (acks.view(np.uint8) == cases.FILL).all(), over
        assert opts.tobytes() == keep_opts.tobytes() and (count == 0xA5A5A5A5A5A5A5A5).all(), over
    assert lib.rxg_ack_plan_host(None) == -EINVAL
    # NULL arrays are fine where their cap is 0
    segs, acks = wsegs.copy(), wacks.copy()
    count = np.zeros(4, np.uint64)
    b, keep = plan_args(s, segs, acks, None, count, segs=None, acks=None, cap=0)
    assert lib.rxg_ack_plan_host(C.byref(b)) == 0 and count.tolist() == [40, 0, 0, 0]


def test_binding_wrapper_equals_the_model():
    s = cases.combo_sets()[1]
    a = s.args
    opts = s.opts_in()
    segs, acks, count = rxg.ack_plan_host(s.order, s.trains, s.train_count, s.n, s.ntcb, s.state, s.rxopts, a["tsval_now"],
                                          a["ip_id0"], a["opt_plain"], a["opt_base"], a["opt_cap"], opts, a["cap"])
    wsegs, wacks, wcount, blocks = s.model()
    k = int(count[0])
    assert count.tolist() == wcount.tolist() and segs[:k].tobytes() == wsegs.tobytes() and acks[:k].tobytes() == wacks.tobytes()
    assert all(opts[i] == b for i, b in blocks.items())


# ----------------------------------------------- 2. the model against the reference ---
@pytest.mark.parametrize("seed", range(4))
def test_acks_against_the_reference_window(seed):
    """Seeded multi-flow bursts: every LIVE flow's segments through the reference's PushData with
    cur_seq as given.  An ADVANCES flow's ACK carries the window's final ptcb->ack -- the value of
    the last in-order delivery; a DUP flow's first train delivers nothing in order."""
    rng = np.random.default_rng(seed)
    nflows, n = 12, 500
    r = ftc.runs(rng.integers(0, nflows, n), seed, p_cont=0.85, p_fin=0.03, datalen=rng.integers(1, 900, n))
    first = {}
    for t, q in zip(r["c"]["tcb_idx"].tolist(), r["seq"].tolist()):
        first.setdefault(t, q)
    cur = {t: (q - 7 * (t % 3 == 0)) & 0xFFFFFFFF for t, q in first.items()}                 # every third flow: a gap of 7 bytes
    b = tpc.build(f"window {seed}", r, nflows, cur=cur, seed=seed)
    order, trains, count = b.trains(rxg.REC48)
    st = cases.states(nflows, seed)
    st["flags"] |= rxg.AS_LIVE
    st["rcv_ack"] = [cur.get(t, 0) for t in range(nflows)]                                    # ptcb->ack before the burst
    segs, acks, cnt, _ = ref.plan(order, trains, count, n, nflows, st)
    assert cnt[0] == len(first) and cnt[1] == cnt[2] == 0
    adv = dup = 0
    frames = b.frames()
    for a in acks:
        t = int(a["tcb_idx"])
        h = trains[int(a["flags_train"]) >> 8]
        assert int(h["tcb_idx"]) == t
        w = window.ReceiveWindow(cur=cur[t])
        seg = order[int(h["first"]):int(h["first"]) + int(h["nseg"])].tolist()
        out, last_ack = [], None
        for i in seg:
            f = frames[i]
            rc, ack = window.push_data(w, int(r["seq"][i]), int(r["c"]["datalen"][i]), f[34:], f[46],
                                       int(r["c"]["tcp_flags"][i]), out)
            if rc == 0:
                last_ack = ack
        if int(a["flags_train"]) & rxg.ACK_ADVANCES:
            assert len(out) == len(seg) and last_ack == int(a["ack"]), t
            assert bool(int(a["flags_train"]) & rxg.ACK_FIN) == bool(int(r["c"]["tcp_flags"][seg[-1]]) & 1)
            adv += 1
        else:
            assert int(a["flags_train"]) & rxg.ACK_DUP and not out and int(a["ack"]) == cur[t], t
            dup += 1
    assert adv >= 4 and dup >= 3


def test_ack_frame_is_sendtcpdatas_and_verifies():
    """opt_plain 0, no timestamps: the frame built from the model's descriptor is the 54 bytes
    sendtcpdata(ptcb, NULL, 0) writes (tcp_out.c:157-207), and the rx oracle sums both checksums
    to 0; with timestamps the option block rides between header and (no) payload."""
    s = cases.wrap_set()
    segs, acks, count, blocks = s.model()
    opts = s.opts_in()[:s.args["opt_cap"]].copy()
    for k, b in blocks.items():
        opts[k] = b
    flows = txbuild_ref.make_flows(s.ntcb)
    off = (np.arange(len(segs)) * 2).astype(np.uint32)
    plain = segs.copy()
    plain["reserved"] = 0
    for sg, table in ((plain, opts), (segs, opts)):
        pool, lens, stats = oref.build(np.zeros(16, np.uint8), flows, sg, table, off, 2 * len(sg))
        assert stats.tolist() == [len(sg), 0]
        for i, g in enumerate(sg):
            k = int(g["reserved"])
            O = int(table[k - 1]["len"]) if k else 0
            f = pool[int(off[i]) * 64:int(off[i]) * 64 + int(lens[i])].tobytes()
            fl = flows[int(g["flow"])]
            assert len(f) == 54 + O
            assert f[12:14] == b"\x08\x00" and f[14] == 0x45 and f[16:18] == (40 + O).to_bytes(2, "big") and f[23] == 6
            assert f[18:20] == int(g["ip_id"]).to_bytes(2, "little")                             # ip.c:106, unswapped
            assert f[34:36] == int(fl["dport"]).to_bytes(2, "big") and f[36:38] == int(fl["sport"]).to_bytes(2, "big")
            assert f[38:42] == int(g["seq"]).to_bytes(4, "big")                                  # sent_seq = htonl(next_seq)
            assert f[42:46] == int(g["ack"]).to_bytes(4, "big")                                  # recv_ack = htonl(ptcb->ack)
            assert f[46] == (5 + O // 4) << 4 and f[47] == rxg.TCP_FLAG_ACK
            assert f[48:50] == (12000).to_bytes(2, "little") and f[52:54] == b"\0\0"             # rx_win 12000 unswapped, urp 0
            assert f[54:] == bytes(table[k - 1]["bytes"][:O]) if k else len(f) == 54
        tcb, live = txbuild_ref_peer(flows)
        recs = oracle.rx_batch(pool, off, lens, tcb, live)[0]["c"]
        assert (recs["verdict"] == rxg.V_DISPATCH).all() and (recs["ip_cksum"] == 0).all() and (recs["tcp_cksum"] == 0).all()
        assert recs["tcb_idx"].tolist() == sg["flow"].tolist() and (recs["datalen"] == 0).all()


def txbuild_ref_peer(flows):
    t = np.zeros(len(flows), dtype=rxg.TCB_DTYPE)
    t["dport"], t["sport"] = flows["sport"], flows["dport"]
    t["ipv4_dst"] = flows["ipv4_src"].byteswap()
    t["ipv4_src"] = flows["ipv4_dst"].byteswap()
    t["state"] = rxg.TCP_ESTABLISHED
    t["identifier"] = 1 + np.arange(len(flows))
    return t, np.ones(len(flows), np.uint8)


# ------------------------------------------------------- 3. layout, header, exports ---
PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "rxg.h"
int main(void) {
    printf("dev %zu\n", sizeof(rxg_dev_ack_plan));
    printf("state %zu\n", offsetof(rxg_dev_ack_plan, state));
    printf("ip_id0 %zu\n", offsetof(rxg_dev_ack_plan, ip_id0));
    printf("opts %zu\n", offsetof(rxg_dev_ack_plan, opts));
    printf("count %zu\n", offsetof(rxg_dev_ack_plan, count));
    printf("st %zu\n", sizeof(rxg_ack_state) * 256 + offsetof(rxg_ack_state, win_raw));
    printf("ack %zu\n", sizeof(rxg_ack) * 256 + offsetof(rxg_ack, flags_train));
    printf("bits %u\n", RXG_AS_LIVE | RXG_AS_TS << 4 | RXG_ACK_ADVANCES << 8 | RXG_ACK_DUP << 12 | RXG_ACK_FIN << 16 | RXG_ACK_NO_OPT << 20);
    return 0;
}
'''


def test_struct_layout_by_c_probe(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", INC, str(tmp_path / "probe.c"), "-o",
                    str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    d = rxg.DevAckPlan
    assert got["dev"] == C.sizeof(d) == 128
    for f in ("state", "ip_id0", "opts", "count"):
        assert got[f] == getattr(d, f).offset, f
    assert got["st"] == 16 * 256 + rxg.ACK_STATE_DTYPE.fields["win_raw"][1]
    assert got["ack"] == 16 * 256 + rxg.ACK_DTYPE.fields["flags_train"][1]
    assert got["bits"] == (rxg.AS_LIVE | rxg.AS_TS << 4 | rxg.ACK_ADVANCES << 8 | rxg.ACK_DUP << 12 | rxg.ACK_FIN << 16 |
                           rxg.ACK_NO_OPT << 20)


def test_entry_points_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "rxg.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
    out = subprocess.run(["nm", "-D", "--defined-only", rxg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (\w+)", out))
    kh = open(os.path.join(CSRC, "rxg_kernels.h")).read()
    assert int(re.search(r"kAkTile = (\d+)", kh).group(1)) == rxg.ACK_PLAN_TILE
    assert int(re.search(r"kAkScanLanes = (\d+)", kh).group(1)) == rxg.ACK_PLAN_SCAN_TILES
    assert rxg.load_library().rxg_abi_version() == 2


# ----------------------------------------------------- 4. the host form stand-alone ---
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_host_function_standalone(tmp_path, san):
    """Every small set and the three T = 257 shapes, each array in a heap block of exactly its size:
    state has ntcb entries (no poison behind it), order cap_seg, rxopts n, opts opt_cap."""
    exe = tmp_path / "ackplan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *san, "-I", INC,
                    os.path.join(ROOT, "tests", "ackplan_check.cpp"), os.path.join(CSRC, "rxg_ackplan.cpp"),
                    os.path.join(CSRC, "rxg_txopt.cpp"), os.path.join(CSRC, "rxg_txplan.cpp"), "-o", str(exe)], check=True)
    jobs = cases.small_sets() + [s for s in cases.size_sets() if s.name.startswith("T=257")]
    blob, want = bytearray(struct.pack("<Q", len(jobs))), bytearray()
    for s in jobs:
        a = s.args
        order, trains = s.order[:a["cap_seg"]], s.trains[:a["cap_trains"]]
        blob += struct.pack("<14Q", len(order), len(trains), s.n, s.ntcb, s.rxopts is not None, a["tsval_now"], a["ip_id0"],
                            a["opt_plain"], a["opt_base"], a["opt_cap"], s.use_opts, a["cap"], a["cap_seg"], a["cap_trains"])
        blob += order.tobytes() + trains.tobytes() + s.train_count.tobytes() + s.state[:s.ntcb].tobytes()
        if s.rxopts is not None:
            assert len(s.rxopts) == s.n
            blob += s.rxopts.tobytes()
        if s.use_opts:
            blob += s.const.tobytes()
        (wsegs, wacks, wopts, wcount), _ = cases.expect(s)
        want += wsegs[:a["cap"]].tobytes() + wacks[:a["cap"]].tobytes()
        if s.use_opts:
            want += wopts[:a["opt_cap"]].tobytes()
        want += wcount.tobytes()
    (tmp_path / "in.bin").write_bytes(bytes(blob))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0 and f"ackplan ok {len(jobs)}" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr
    assert (tmp_path / "out.bin").read_bytes() == bytes(want)
