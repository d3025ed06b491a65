#!/usr/bin/env python3
"""Per-flow summary micro-benchmark (rxg_flow_sums_dev).  2^20 DISPATCH frames of
64 B or 1 500 B at a fixed stride, every one a bare ACK without options, spread at random over 1,
1 000 or 65 536 flows of a 65 536-entry table, with crafted 8- or 48-byte records.  One run times,
in interleaved rounds over `--sets` rotating sets of buffers on the context's stream and between
two rxg_event_* records each,
  a  rxg_flow_sums_dev (four launches); fraction of 8 TB/s on its algorithmic bytes: n * record
     size + 16 per counted frame (8-byte records) + 2 n of len + ntcb / 8 of bitmap + 40 per flow
  b  rxg_rx_opts_dev on the same batch: the yardstick for a pass over the records and one line
     per frame
  c  rxg_flow_sums_dev on the first 64 frames of the batch: the launches, the bitmap count, the
     scan and the expansion of one flow, without the accumulation's work
and checks a's output against numpy first.  `--max-blocks` adds contexts whose grids are capped
(the accumulation's grid decides how many waves end with atomics on the one flow).
  python scripts/flowsumbench.py [--n 1048576 --rounds 5 --iters 20 --max-blocks 256,2048]"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--max-blocks", default="", help="comma-separated grid caps to time besides the default")
    args = ap.parse_args()
    import torch

    import flowsum_ref as ref
    import rxg
    assert torch.cuda.is_available(), "flowsumbench needs a GPU"
    dev = torch.device("cuda:0")
    n = args.n
    engines = [("default", rxg.Engine(0))] + [(f"max_blocks {k}", rxg.Engine(0, max_blocks=int(k)))
                                              for k in args.max_blocks.split(",") if k]
    eng = engines[0][1]

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    def timed(e, fn, sets):
        out = []
        for _ in range(args.rounds):
            evs = [(e.event(), e.event()) for _ in range(args.iters)]
            for i, (a, b) in enumerate(evs):
                e.record(a)
                fn(e, sets[i % len(sets)])
                e.record(b)
            e.sync()
            out.append(float(np.median([e.elapsed_ms(a, b) for a, b in evs])) * 1e3)
            for a, b in evs:
                e.event_destroy(a)
                e.event_destroy(b)
        return out

    def row(**kw):
        us = kw.pop("rounds_us")
        med = float(np.median(us))
        print(json.dumps(dict(us=round(med, 1), rounds_us=[round(x, 1) for x in us],
                              spread_pct=round(100 * (max(us) - min(us)) / med, 1), **kw)), flush=True)
        return med

    for flen in (64, 1500):
        stride64 = (flen + 63) // 64
        for nflows in (1, 1000, 65536):
            for kind in (rxg.REC8, rxg.REC48):
                sets = []
                for k in range(args.sets):
                    rng = np.random.default_rng(1000 * k + nflows)
                    tcb = rng.integers(0, nflows, n)
                    seq, ack = rng.integers(0, 2**32, n, dtype=np.uint64), rng.integers(0, 2**32, n, dtype=np.uint64)
                    r48 = np.zeros(n, rxg.REC48_DTYPE)
                    c = r48["c"]
                    c["tcb_idx"], c["state"], c["tcp_flags"], c["flags"] = tcb, 4, 0x10, 3
                    r48["c"] = c
                    r48["seq"], r48["ack"] = seq, ack
                    recs = r48 if kind == rxg.REC48 else rxg.rec8_pack(np.ascontiguousarray(r48["c"]))
                    arena = torch.randint(0, 256, (n, stride64 * 64), dtype=torch.uint8, device=dev)
                    arena[:, 46] = 0x50                      # no options: the yardstick walks nothing
                    head = np.zeros((n, 8), np.uint8)        # seq and ack where the 8-byte records' pass reads them
                    head[:, :4] = seq.astype(">u4").view(np.uint8).reshape(n, 4)
                    head[:, 4:] = ack.astype(">u4").view(np.uint8).reshape(n, 4)
                    arena[:, 38:46] = torch.from_numpy(head).to(dev)
                    s = dict(arena=arena, len=dev_of(np.full(n, flen, np.uint16)), recs=dev_of(recs),
                             out=torch.zeros(NTCB * 40, dtype=torch.uint8, device=dev),
                             count=torch.zeros(3, dtype=torch.int64, device=dev),
                             opts=torch.zeros(n * 16, dtype=torch.uint8, device=dev))
                    if k == 0:
                        want, wcount = ref.summaries(recs, kind, NTCB, None, 0) if kind == rxg.REC48 else \
                            ref.summaries(r48, rxg.REC48, NTCB, None, 0)
                        s["want"] = (want, wcount)
                    sets.append(s)
                torch.cuda.synchronize()

                def flow_sums(e, s, m=n):
                    e.flow_sums_dev(s["recs"].data_ptr(), kind, m, NTCB, s["out"].data_ptr(), NTCB, s["count"].data_ptr(),
                                    frames=s["arena"].data_ptr(), lens=s["len"].data_ptr(), slot0=0, stride64=stride64)

                def rx_opts(e, s):
                    e.rx_opts_dev(s["arena"].data_ptr(), s["len"].data_ptr(), n, s["recs"].data_ptr(), kind,
                                  s["opts"].data_ptr(), off64=None, slot0=0, stride64=stride64)

                flow_sums(eng, sets[0])
                eng.sync()
                want, wcount = sets[0]["want"]
                assert sets[0]["count"].cpu().numpy().tolist() == wcount.tolist()
                got = sets[0]["out"].cpu().numpy()[:len(want) * 40].view(rxg.FLOW_SUM_DTYPE)
                assert got.tobytes() == want.tobytes(), "rxg_flow_sums_dev differs from numpy"
                alg = n * kind + (16 * n + 2 * n if kind != rxg.REC48 else 0) + NTCB // 8 + 40 * len(want)
                base = dict(frame_len=flen, flows=nflows, rec_kind=kind, n=n)
                for name, e in engines:
                    for s in sets:                            # warm every buffer on this context
                        flow_sums(e, s)
                        rx_opts(e, s)
                    e.sync()
                    ta, tb = timed(e, flow_sums, sets), timed(e, rx_opts, sets)
                    tc = timed(e, lambda e_, s_: flow_sums(e_, s_, 64), sets)
                    a = row(variant="a_flow_sums_dev", grid=name, rounds_us=ta, alg_bytes=alg, **base)
                    b = row(variant="b_rx_opts_dev", grid=name, rounds_us=tb, **base)
                    c_ = row(variant="c_flow_sums_dev_64_frames", grid=name, rounds_us=tc, **base)
                    print(json.dumps(dict(grid=name, ratio_a_to_b=round(a / b, 2), frac_8TBs=round(alg / (a * 1e-6) / 8e12, 4),
                                          acc_part_us=round(a - c_, 1), **base)), flush=True)
                del sets
                torch.cuda.empty_cache()
    for _, e in engines:
        e.close()


if __name__ == "__main__":
    main()
