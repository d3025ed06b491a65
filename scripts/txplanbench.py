#!/usr/bin/env python3
"""Device planner micro-benchmark (rxg_tx_plan_dev).  Workloads of 2^20 segments
at mss 1 460:
  A_plain  64 KiB sends (45 segments each)
  A_ts     64 KiB sends that carry the 12-byte timestamp block (46 segments each)
  B        2^20 one-segment sends
One run times, in interleaved rounds over `--sets` rotating sets of buffers on one stream,
  old  the route there was before: rxg_tx_plan_opt into pinned host memory (host part), then
       rxg_memcpy_h2d of the descriptors (copy part, wall clock around a stream sync)
  new  rxg_memcpy_h2d of the sends (and send_opt) from pinned host memory, then rxg_tx_plan_dev
       (wall clock around a stream sync); its launches alone between two device events give the
       fraction of 8 TB/s on the algorithmic bytes: per send 40 (+ 4 with send_opt) read and
       8 + 4 written, per segment 32 written
Both routes' descriptors are compared byte for byte on every set first.  Each workload runs in a
child process of its own under a time limit; the first failure ends the run.
  python scripts/txplanbench.py [--segs 1048576 --rounds 5 --iters 10 --limit 300]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dpdk-tcpipstack_amd")]

MSS = 1460
WORKLOADS = {"A_plain": dict(bytes=65536, block=0), "A_ts": dict(bytes=65536, block=1), "B": dict(bytes=MSS, block=0)}


def worker(args):
    import torch

    import rxg
    assert torch.cuda.is_available(), "txplanbench needs a GPU"
    w = WORKLOADS[args.worker]
    eng = rxg.Engine(0)
    lib = rxg.load_library()
    ts = torch.cuda.Stream(torch.device("cuda:0"))  # (not the null stream: rxg takes that as the context's own)
    st = ts.cuda_stream
    table = np.array([rxg.tx_opt_timestamp(1, 2)], dtype=rxg.TX_OPT_DTYPE)
    m = MSS - (12 if w["block"] else 0)
    per = -(-w["bytes"] // m)
    nsends = -(-args.segs // per)
    n = nsends * per
    d_opts = eng.to_device(table)
    sets = []
    for k in range(args.sets):
        r = np.random.default_rng(90 + k)
        sends = np.zeros(nsends, dtype=rxg.TX_SEND_DTYPE)
        sends["flow"] = r.integers(0, 10000, nsends)
        sends["next_seq"] = r.integers(0, 1 << 32, nsends, dtype=np.uint64)
        sends["ack"] = r.integers(0, 1 << 32, nsends, dtype=np.uint64)
        sends["src_off"] = np.arange(nsends, dtype=np.uint64) * w["bytes"]
        sends["bytes"], sends["tcp_flags"], sends["win_raw"] = w["bytes"], rxg.TCP_FLAG_ACK | rxg.TCP_FLAG_PSH, 12000
        sends["ip_id0"] = r.integers(0, 1 << 16, nsends)
        so = np.full(nsends, w["block"], np.uint32) if w["block"] else None
        assert rxg.tx_plan_count(sends, MSS, so, table) == n
        s = dict(h_sends=eng.pinned(nsends * 40), h_so=eng.pinned(nsends * 4), h_segs=eng.pinned(n * 32),
                 d_sends=eng.alloc(nsends * 40), d_so=eng.alloc(nsends * 4), d_old=eng.alloc(n * 32),
                 d_new=eng.alloc(n * 32), d_first=eng.alloc((nsends + 1) * 8), d_next=eng.alloc(nsends * 4),
                 d_count=eng.alloc(16), h_next=np.zeros(nsends, np.uint32), so=so is not None)
        s["h_sends"].np[:nsends * 40] = sends.view(np.uint8).reshape(-1)
        if so is not None:
            s["h_so"].np[:nsends * 4] = so.view(np.uint8)
        sets.append(s)

    def old_route(s, times=None):
        t0 = time.perf_counter()
        got = lib.rxg_tx_plan_opt(s["h_sends"].ptr, nsends, MSS, s["h_so"].ptr if s["so"] else None, table.ctypes.data,
                                  len(table), s["h_segs"].ptr, n, s["h_next"].ctypes.data)
        t1 = time.perf_counter()
        assert got == n, got
        eng.h2d(s["d_old"].ptr, s["h_segs"].ptr, n * 32, stream=st)
        eng.stream_sync(st)
        t2 = time.perf_counter()
        if times is not None:
            times.append((t1 - t0, t2 - t1))

    def plan(s):
        eng.tx_plan_dev(s["d_sends"].ptr, nsends, MSS, s["d_new"].ptr, n, s["d_first"].ptr, s["d_count"].ptr,
                        send_opt=s["d_so"].ptr if s["so"] else None, opts=d_opts.ptr, nopts=len(table),
                        next_seq=s["d_next"].ptr, stream=st)

    def new_route(s, times=None):
        t0 = time.perf_counter()
        eng.h2d(s["d_sends"].ptr, s["h_sends"].ptr, nsends * 40, stream=st)
        if s["so"]:
            eng.h2d(s["d_so"].ptr, s["h_so"].ptr, nsends * 4, stream=st)
        plan(s)
        eng.stream_sync(st)
        if times is not None:
            times.append(time.perf_counter() - t0)

    for k, s in enumerate(sets):  # both routes give the same descriptors, on every set
        lib.rxg_memset_dev(eng.ctx, s["d_new"].ptr, 0xA5, n * 32, st)
        new_route(s)
        old_route(s)
        a, b = s["d_new"].download(np.uint8, n * 32, stream=st), s["d_old"].download(np.uint8, n * 32, stream=st)
        assert s["d_count"].download(np.uint64, 2, stream=st).tolist() == [n, 0]
        assert np.array_equal(a, b), f"set {k}: rxg_tx_plan_dev and rxg_tx_plan_opt differ"
        assert np.array_equal(s["d_next"].download(np.uint32, nsends, stream=st), s["h_next"])

    new_us, old_host, old_copy, kern_us = [], [], [], []
    e0, e1 = eng.event(), eng.event()
    for _ in range(args.rounds):
        tn, to = [], []
        for i in range(args.iters):
            new_route(sets[i % len(sets)], tn)
            old_route(sets[i % len(sets)], to)
        for i in range(args.iters):  # the planner's launches alone, between two device events
            eng.record(e0, st)
            plan(sets[i % len(sets)])
            eng.record(e1, st)
            eng.stream_sync(st)
            kern_us.append(eng.elapsed_ms(e0, e1) * 1e3)
        new_us += [t * 1e6 for t in tn]
        old_host += [t[0] * 1e6 for t in to]
        old_copy += [t[1] * 1e6 for t in to]

    def row(name, us, **kw):
        print(json.dumps(dict(workload=args.worker, variant=name, segs=n, sends=nsends, samples=len(us),
                              min_us=round(min(us), 1), median_us=round(float(np.median(us)), 1),
                              max_us=round(max(us), 1), **kw)), flush=True)
        return float(np.median(us))
    alg = nsends * (40 + (4 if w["block"] else 0) + 8 + 4) + n * 32
    new = row("new_h2d_sends_plus_tx_plan_dev", new_us)
    row("new_tx_plan_dev_launches_only", kern_us, alg_bytes=alg,
        frac_8TBs=round(alg / (float(np.median(kern_us)) * 1e-6) / 8e12, 4))
    old_total = [h + c for h, c in zip(old_host, old_copy)]
    row("old_host_part_tx_plan_opt", old_host)
    row("old_copy_part_h2d_descriptors", old_copy, GBps=round(n * 32 / (float(np.median(old_copy)) * 1e-6) / 1e9, 1))
    old = row("old_total", old_total)
    print(json.dumps(dict(workload=args.worker, new_median_below_old_whole_spread=bool(new < min(old_total)),
                          ratio_old_total_to_new=round(old / new, 1))), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segs", type=int, default=1 << 20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=300, help="seconds each workload's process may take")
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    for name in ("A_plain", "A_ts", "B"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--segs", str(args.segs), "--sets", str(args.sets), "--rounds", str(args.rounds), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(f"txplanbench: workload {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
