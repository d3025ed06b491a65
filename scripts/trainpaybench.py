#!/usr/bin/env python3
"""Train-payload micro-benchmark (rxg_train_payload_dev) on §5.10's batches: 2^20
frames of 64 B or 1 500 B at a fixed stride, every one a data segment of a live flow, spread at
random over 1, 1 000 or 65 536 flows with random seq (every segment a train of its own) -- and
`trains`: 1 000 flows whose segments continue each other in runs of 64 (16 384 trains).  The
frames carry real headers, so the records are rxg_rx_burst_dev's own (8-byte) and
rxg_payload_gather_dev runs on the same burst.  One run times, in interleaved rounds on the
context's stream and between two rxg_event_* records each,
  a  rxg_train_payload_dev (the trains computed before)
  b  rxg_flow_trains_dev + rxg_train_payload_dev
  c  rxg_payload_gather_dev on the same burst
and checks a's output against the numpy model first (--check-n frames of it where n is larger).
  python scripts/trainpaybench.py [--n 1048576 --rounds 3 --iters 10]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dpdk-tcpipstack_amd"), os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-n", type=int, default=1 << 16)
    args = ap.parse_args()
    import torch

    import flowtrain_ref
    import pktgen
    import rxg
    import trainpay_ref as ref
    assert torch.cuda.is_available(), "trainpaybench needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    eng = rxg.Engine(0)

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    def timed(fn):
        out = []
        for _ in range(args.rounds):
            evs = [(eng.event(), eng.event()) for _ in range(args.iters)]
            for a, b in evs:
                eng.record(a)
                fn()
                eng.record(b)
            eng.sync()
            out.append(float(np.median([eng.elapsed_ms(a, b) for a, b in evs])) * 1e3)
            for a, b in evs:
                eng.event_destroy(a)
                eng.event_destroy(b)
        return out

    def row(**kw):
        us = kw.pop("rounds_us")
        med = float(np.median(us))
        print(json.dumps(dict(us=round(med, 1), min_us=round(min(us), 1), max_us=round(max(us), 1), **kw)), flush=True)
        return med

    dst = pktgen.ip4(192, 168, 78, 2)
    shapes = [(flen, nflows, False) for flen in (64, 1500) for nflows in (1, 1000, 65536)] + [(1500, 1000, True)]
    for flen, nflows, in_runs in shapes:
        stride64, dl = (flen + 63) // 64, flen - 54
        rng = np.random.default_rng(nflows + flen)
        tcb, live = rxg.synthetic_tcb_table(nflows)
        ntcb = len(tcb)                                  # (the flows' TCBs and the listener)
        eng.tcb_load(tcb, live)
        eng.tcb_sync()
        # one header per flow (rxg_synth_params' flow numbering), the IP checksum valid for this length
        hdr = np.zeros((nflows, 54), np.uint8)
        for f in range(nflows):
            fr = pktgen.frame(src_ip=pktgen.ip4(10, (f >> 16) & 255, (f >> 8) & 255, f & 255), dst_ip=dst,
                              sport=1024 + f % 64511, dport=80, seq=0, ack=1, flags=0x10, payload=bytes(dl), valid_tcp=False)
            hdr[f] = np.frombuffer(fr[:54], np.uint8)
        flow = rng.integers(0, nflows, n)
        if in_runs:                                      # a flow's k-th segment continues its (k - 1)-th but every 64th
            o = np.argsort(flow, kind="stable")
            rank = np.empty(n, np.int64)
            starts = np.searchsorted(flow[o], np.arange(nflows))
            rank[o] = np.arange(n) - starts[flow[o]]
            base = rng.integers(1, 2**31, (nflows, n // 64 + 2), dtype=np.uint64)
            seq = (base[flow, rank // 64] + (rank % 64).astype(np.uint64) * dl) & 0xFFFFFFFF
        else:
            seq = rng.integers(1, 2**32 - 70000, n, dtype=np.uint64)
        arena = torch.randint(0, 256, (n, stride64 * 64), dtype=torch.uint8, device=dev)
        arena[:, :54] = torch.from_numpy(hdr).to(dev)[torch.from_numpy(flow).to(dev)]
        arena[:, 38:42] = torch.from_numpy(seq.astype(">u4").view(np.uint8).reshape(n, 4).copy()).to(dev)
        lens = dev_of(np.full(n, flen, np.uint16))
        off = dev_of((np.arange(n) * stride64).astype(np.uint32))
        recs = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
        span = (dl + 15) // 16 * 16
        cap = n * span
        order = torch.zeros(n, dtype=torch.int32, device=dev)
        trains = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
        count = torch.zeros(4, dtype=torch.int64, device=dev)
        out = torch.zeros(cap, dtype=torch.uint8, device=dev)
        msgs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        tmsgs = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        used = torch.zeros(1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()

        def burst(m=n):
            eng.rx_burst_dev(arena.data_ptr(), off.data_ptr(), lens.data_ptr(), m, recs.data_ptr(), rxg.REC8)

        def flow_trains(m=n):
            eng.flow_trains_dev(recs.data_ptr(), rxg.REC8, m, ntcb, order.data_ptr(), n, trains.data_ptr(), n,
                                count.data_ptr(), frames=arena.data_ptr(), lens=lens.data_ptr(), off64=off.data_ptr())

        def train_payload(m=n):
            eng.train_payload_dev(arena.data_ptr(), lens.data_ptr(), m, recs.data_ptr(), rxg.REC8, order.data_ptr(), n,
                                  trains.data_ptr(), n, count.data_ptr(), out.data_ptr(), cap, msgs.data_ptr(),
                                  tmsgs.data_ptr(), used.data_ptr(), off64=off.data_ptr())

        def both():
            flow_trains()
            train_payload()

        def gather():
            eng.payload_gather_dev(out.data_ptr(), cap, msgs.data_ptr(), used.data_ptr())

        # the check, on the first check-n frames: the device's bytes against the numpy model
        m = min(n, args.check_n)
        burst(m)
        flow_trains(m)
        train_payload(m)
        eng.sync()
        r8 = recs.cpu().numpy()[:m * 8]
        c16 = rxg.rec8_expand(r8.view(rxg.REC8_DTYPE))
        assert (c16["verdict"] == rxg.V_DISPATCH).all() and (c16["datalen"] == dl).all(), "the crafted frames are not DISPATCH"
        pool = arena[:m].cpu().numpy().reshape(-1)
        frames = [pool[i * stride64 * 64:i * stride64 * 64 + flen].tobytes() for i in range(m)]
        worder, wtrains, wcount = flowtrain_ref.trains(r8, rxg.REC8, ntcb, frames)
        full = int(ref.pad16(wtrains["bytes"].astype(np.int64)).sum())
        wa, wm, wtm, wused = ref.gather(pool, (np.arange(m) * stride64).astype(np.uint32), np.full(m, flen, np.uint16), r8,
                                        rxg.REC8, worder, wtrains, wcount, m, m, 0, np.zeros(full, np.uint8), cap)
        assert int(wcount[0]) == m and int(used.cpu()[0]) == wused == full
        assert out[:full].cpu().numpy().tobytes() == wa.tobytes(), "rxg_train_payload_dev differs from numpy (arena)"
        assert msgs.cpu().numpy()[:m * 16].tobytes() == wm.tobytes(), "rxg_train_payload_dev differs from numpy (msgs)"
        assert tmsgs.cpu().numpy()[:len(wtm) * 16].tobytes() == wtm.tobytes(), "rxg_train_payload_dev differs from numpy (tmsgs)"
        burst()
        flow_trains()
        both()
        gather()
        eng.sync()
        ntrains = int(count.cpu()[1])
        base = dict(frame_len=flen, flows=nflows, n=n, shape="trains" if in_runs else "random", trains=ntrains,
                    payload_bytes=n * dl)
        ta, tb, tc = timed(train_payload), timed(both), timed(gather)
        a = row(variant="a_train_payload_dev", rounds_us=ta, **base)
        b = row(variant="b_flow_trains_dev_plus_train_payload_dev", rounds_us=tb, **base)
        c_ = row(variant="c_payload_gather_dev", rounds_us=tc, **base)
        floor_us = 2 * n * dl / 8e12 * 1e6
        print(json.dumps(dict(ratio_a_to_c=round(a / c_, 2), ratio_b_to_c=round(b / c_, 2),
                              floor_us_at_8TBs=round(floor_us, 1), floor_share_of_a=round(floor_us / a, 3), **base)),
              flush=True)
        del arena, out, msgs, tmsgs, order, trains, recs
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
