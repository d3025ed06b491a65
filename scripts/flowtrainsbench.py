#!/usr/bin/env python3
"""Flow-train micro-benchmark (rxg_flow_trains_dev), on scripts/flowsumbench.py's
batches: 2^20 DISPATCH frames of 64 B or 1 500 B at a fixed stride, every one a data segment,
spread at random over 1, 1 000 or 65 536 flows of a 65 536-entry table, with crafted 8- or
48-byte records -- and a seventh shape, `trains`: 1 000 flows arriving in runs of 64 contiguous
segments.  One run times, in interleaved rounds over `--sets` rotating sets of buffers on the
context's stream and between two rxg_event_* records each,
  a  rxg_flow_trains_dev (7 + 3 * passes launches; the table takes 2 passes)
  b  rxg_flow_sums_dev on the same batch: one pass over the same records, one line per counted
     frame, a result per flow
  c  rxg_flow_trains_dev on the first 64 frames of the batch: the launch floor
and checks a's output against the numpy model first.
  python scripts/flowtrainsbench.py [--n 1048576 --rounds 3 --iters 20]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dpdk-tcpipstack_amd"), os.path.join(ROOT, "tests")]

NTCB = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch

    import flowtrain_ref as ref
    import rxg
    assert torch.cuda.is_available(), "flowtrainsbench needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    eng = rxg.Engine(0)

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    def timed(fn, sets):
        out = []
        for _ in range(args.rounds):
            evs = [(eng.event(), eng.event()) for _ in range(args.iters)]
            for i, (a, b) in enumerate(evs):
                eng.record(a)
                fn(sets[i % len(sets)])
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

    shapes = [(flen, nflows, kind, False) for flen in (64, 1500) for nflows in (1, 1000, 65536)
              for kind in (rxg.REC8, rxg.REC48)]
    shapes += [(1500, 1000, rxg.REC8, True), (1500, 1000, rxg.REC48, True)]
    for flen, nflows, kind, in_runs in shapes:
        stride64 = (flen + 63) // 64
        dl = flen - 54
        sets = []
        for k in range(args.sets):
            rng = np.random.default_rng(1000 * k + nflows)
            if in_runs:                                  # runs of 64 contiguous segments per flow
                tcb = np.repeat(rng.integers(0, nflows, (n + 63) // 64), 64)[:n]
                start = np.repeat(rng.integers(1, 2**31, (n + 63) // 64, dtype=np.uint64), 64)[:n]
                seq = (start + (np.arange(n, dtype=np.uint64) % 64) * dl) & 0xFFFFFFFF
            else:
                tcb = rng.integers(0, nflows, n)
                seq = rng.integers(0, 2**32, n, dtype=np.uint64)
            ack = rng.integers(0, 2**32, n, dtype=np.uint64)
            r48 = np.zeros(n, rxg.REC48_DTYPE)
            c = r48["c"]
            c["tcb_idx"], c["state"], c["tcp_flags"], c["flags"], c["datalen"] = tcb, 4, 0x10, 3, dl
            r48["c"] = c
            r48["seq"], r48["ack"] = seq, ack
            recs = r48 if kind == rxg.REC48 else rxg.rec8_pack(np.ascontiguousarray(r48["c"]))
            arena = torch.randint(0, 256, (n, stride64 * 64), dtype=torch.uint8, device=dev)
            head = np.zeros((n, 8), np.uint8)            # seq and ack where the 8-byte records' passes read them
            head[:, :4] = seq.astype(">u4").view(np.uint8).reshape(n, 4)
            head[:, 4:] = ack.astype(">u4").view(np.uint8).reshape(n, 4)
            arena[:, 38:46] = torch.from_numpy(head).to(dev)
            s = dict(arena=arena, len=dev_of(np.full(n, flen, np.uint16)), recs=dev_of(recs),
                     order=torch.zeros(n, dtype=torch.int32, device=dev),
                     trains=torch.zeros(n * 32, dtype=torch.uint8, device=dev),
                     count=torch.zeros(4, dtype=torch.int64, device=dev),
                     sums=torch.zeros(NTCB * 40, dtype=torch.uint8, device=dev),
                     scount=torch.zeros(3, dtype=torch.int64, device=dev))
            if k == 0:
                s["want"] = ref.trains(r48, rxg.REC48, NTCB)
            sets.append(s)
        torch.cuda.synchronize()

        def flow_trains(s, m=n):
            eng.flow_trains_dev(s["recs"].data_ptr(), kind, m, NTCB, s["order"].data_ptr(), n, s["trains"].data_ptr(), n,
                                s["count"].data_ptr(), frames=s["arena"].data_ptr(), lens=s["len"].data_ptr(), slot0=0,
                                stride64=stride64)

        def flow_sums(s):
            eng.flow_sums_dev(s["recs"].data_ptr(), kind, n, NTCB, s["sums"].data_ptr(), NTCB, s["scount"].data_ptr(),
                              frames=s["arena"].data_ptr(), lens=s["len"].data_ptr(), slot0=0, stride64=stride64)

        flow_trains(sets[0])
        eng.sync()
        worder, wtrains, wcount = sets[0]["want"]
        assert sets[0]["count"].cpu().numpy().tolist() == wcount.tolist()
        assert sets[0]["order"].cpu().numpy().view(np.uint32)[:len(worder)].tobytes() == worder.tobytes()
        got = sets[0]["trains"].cpu().numpy()[:len(wtrains) * 32].view(rxg.FLOW_TRAIN_DTYPE)
        assert got.tobytes() == wtrains.tobytes(), "rxg_flow_trains_dev differs from numpy"
        base = dict(frame_len=flen, flows=nflows, rec_kind=kind, n=n, shape="trains" if in_runs else "random",
                    trains=len(wtrains))
        for s in sets:                                    # warm every buffer
            flow_trains(s)
            flow_sums(s)
        eng.sync()
        ta, tb = timed(flow_trains, sets), timed(flow_sums, sets)
        tc = timed(lambda s_: flow_trains(s_, 64), sets)
        a = row(variant="a_flow_trains_dev", rounds_us=ta, **base)
        b = row(variant="b_flow_sums_dev", rounds_us=tb, **base)
        c_ = row(variant="c_flow_trains_dev_64_frames", rounds_us=tc, **base)
        print(json.dumps(dict(ratio_a_to_b=round(a / b, 2), ratio_a_to_c=round(a / c_, 2), **base)), flush=True)
        del sets
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
