#!/usr/bin/env python3
"""ACK-plan micro-benchmark (rxg_ack_plan_dev) on the train lists §5.10's batches
give: 2^20 data segments spread at random over 1, 1 000 or 65 536 flows with random seq (every
segment a train of its own: 2^20 trains) -- and `trains`: 1 000 flows whose segments continue each
other in runs of 64, a flow's remainder a train too (16 878 trains).  The call is a pure function of the trains, so the lists are
written directly (what rxg_flow_trains_dev writes for such a burst); every flow is LIVE, every other
one negotiated timestamps, every flow's first train is HEAD, rxopts carry a timestamp.  One run
times, in interleaved rounds,
  a  rxg_ack_plan_dev on the list (between two rxg_event_* records on the context's stream)
  b  rxg_ack_plan_dev on the list's first 64 trains: the call's launch floor
  c  rxg_ack_plan_host on the same list, one core (wall clock)
and checks a's segs, acks, option blocks and count against c's first.
  python scripts/ackplanbench.py [--n 1048576 --rounds 3 --iters 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dpdk-tcpipstack_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    import torch

    import rxg
    assert torch.cuda.is_available(), "ackplanbench needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    eng = rxg.Engine(0)

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    def device_us(fn):
        evs = [(eng.event(), eng.event()) for _ in range(args.iters)]
        for a, b in evs:
            eng.record(a)
            fn()
            eng.record(b)
        eng.sync()
        us = float(np.median([eng.elapsed_ms(a, b) for a, b in evs])) * 1e3
        for a, b in evs:
            eng.event_destroy(a)
            eng.event_destroy(b)
        return us

    def row(**kw):
        us = kw.pop("rounds_us")
        med = float(np.median(us))
        print(json.dumps(dict(us=round(med, 1), min_us=round(min(us), 1), max_us=round(max(us), 1), **kw)), flush=True)
        return med

    for nflows, run in ((1, 1), (1000, 1), (65536, 1), (1000, 64)):
        rng = np.random.default_rng(nflows + run)
        flow = np.sort(rng.integers(0, nflows, n))
        rank = np.arange(n) - np.searchsorted(flow, flow)            # a segment's rank inside its flow
        starts = np.nonzero(rank % run == 0)[0]                      # a train every `run` segments of a flow
        T = len(starts)
        trains = np.zeros(T, dtype=rxg.FLOW_TRAIN_DTYPE)
        trains["tcb_idx"] = flow[starts]
        trains["first"] = starts
        trains["nseg"] = np.diff(np.r_[starts, n])
        trains["seq"] = rng.integers(1, 1 << 31, T)
        trains["bytes"] = trains["nseg"].astype(np.uint64) * 1446
        trains["next_ack"] = (trains["seq"] + trains["bytes"]) & 0xFFFFFFFF
        trains["flags"] = np.where(rank[starts] == 0, rxg.FTR_HEAD | rxg.FTR_FLOW_FIRST, 0)
        order = rng.permutation(n).astype(np.uint32)
        tcount = np.array([n, T, 0, 0], np.uint64)
        state = np.zeros(nflows, dtype=rxg.ACK_STATE_DTYPE)
        state["snd_nxt"], state["rcv_ack"], state["ts_recent"] = 1000, 2000, 3000
        state["win_raw"] = 12000
        state["flags"] = rxg.AS_LIVE | np.where(np.arange(nflows) % 2 == 0, rxg.AS_TS, 0)
        rxopts = np.zeros(n, dtype=rxg.RX_OPT_DTYPE)
        rxopts["flags"] = rxg.O_PARSED | rxg.O_TS
        rxopts["tsval"] = 7000 + np.arange(n)
        flows_present = len(np.unique(flow))
        cap, opt_cap = flows_present, 1 + flows_present
        const = np.zeros(1, dtype=rxg.TX_OPT_DTYPE)
        const[0] = rxg.tx_opt_ref_ack()[0]

        d_order, d_trains, d_tcount, d_state, d_rx = (dev_of(x) for x in (order, trains, tcount, state, rxopts))
        d_segs = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        d_acks = torch.zeros(cap * 16, dtype=torch.uint8, device=dev)
        d_opts = torch.zeros(opt_cap * 48, dtype=torch.uint8, device=dev)
        d_opts[:48] = dev_of(const)
        d_count = torch.zeros(4, dtype=torch.int64, device=dev)
        d_tc64 = dev_of(np.array([n, min(64, T), 0, 0], np.uint64))
        torch.cuda.synchronize()

        def plan(tc=d_tcount, cap_trains=T):
            eng.ack_plan_dev(d_order.data_ptr(), n, d_trains.data_ptr(), cap_trains, tc.data_ptr(), n, nflows,
                             d_state.data_ptr(), d_segs.data_ptr(), d_acks.data_ptr(), cap, d_count.data_ptr(),
                             rxopts=d_rx.data_ptr(), tsval_now=0x01020304, ip_id0=0xFFF0, opt_plain=1, opt_base=1,
                             opt_cap=opt_cap, opts=d_opts.data_ptr())

        def floor():
            plan(d_tc64, min(64, T))

        h_opts = np.zeros(opt_cap, dtype=rxg.TX_OPT_DTYPE)
        h_opts[0] = const[0]
        h_segs, h_acks = np.zeros(cap, dtype=rxg.TX_SEG_DTYPE), np.zeros(cap, dtype=rxg.ACK_DTYPE)

        def host():
            t0 = time.perf_counter()
            out = rxg.ack_plan_host(order, trains, tcount, n, nflows, state, rxopts, 0x01020304, 0xFFF0, 1, 1, opt_cap,
                                    h_opts, cap, h_segs, h_acks)
            return (time.perf_counter() - t0) * 1e6, out

        plan()
        eng.sync()
        _, (wsegs, wacks, wcount) = host()
        A = int(wcount[0])
        assert A == flows_present and d_count.cpu().numpy().view(np.uint64).tolist() == wcount.tolist()
        assert d_segs.cpu().numpy().tobytes() == wsegs.tobytes(), "rxg_ack_plan_dev differs from the host form (segs)"
        assert d_acks.cpu().numpy().tobytes() == wacks.tobytes(), "rxg_ack_plan_dev differs from the host form (acks)"
        assert d_opts.cpu().numpy().tobytes() == h_opts.tobytes(), "rxg_ack_plan_dev differs from the host form (opts)"
        ta, tb, tc = [], [], []
        for _ in range(args.rounds):                                 # interleaved: a, b, c in every round
            ta.append(device_us(plan))
            tb.append(device_us(floor))
            tc.append(float(np.median([host()[0] for _ in range(3)])))
        base = dict(flows=nflows, segments=n, trains=T, acks=A, shape="runs of 64" if run > 1 else "random")
        a = row(variant="a_ack_plan_dev", rounds_us=ta, **base)
        b = row(variant="b_ack_plan_dev_64_trains", rounds_us=tb, **base)
        c_ = row(variant="c_ack_plan_host", rounds_us=tc, **base)
        bytes_alg = T * 16 + 2 * A * 16 + A * 48 + (A // 2) * (4 + 16 + 48) + 3 * ((T + 255) // 256) * 16
        print(json.dumps(dict(ratio_a_to_floor=round(a / b, 2), ratio_host_to_a=round(c_ / a, 2), algorithmic_bytes=bytes_alg,
                              us_at_8TBs=round(bytes_alg / 8e12 * 1e6, 2), **base)), flush=True)
        del d_order, d_trains, d_rx, d_segs, d_acks, d_opts
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
