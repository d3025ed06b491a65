#!/usr/bin/env python3
"""Reset build micro-benchmark (rxg_tx_reset_dev).  Two workloads of 2^20
synthetic frames each, classified by a real rxg_rx_burst_dev (RXG_REC8 records):
  flood   64 B frames to a port nobody owns: every frame is RST_NOPCB (a SYN flood / port scan)
  sparse  1 500 B frames, 1 % of the flows without a TCB: 1 % of the frames RST_NOPCB
One run times, in interleaved rounds over `--sets` rotating sets of buffers on one stream,
  a  rxg_tx_reset_dev (count + scan + build launches), fraction of 8 TB/s on its algorithmic
     bytes: 2 * n * 8 (records, read twice) + per reset 64 + 64 + 4
  b  the only device route there was before it: the records copied to the host, the offenders
     picked there, their first lines gathered on the device (torch) and copied to the host,
     one zero-length rxg_tx_build_dev descriptor and one flow record written per reset on the
     host (numpy, vectorised), copied back, rxg_tx_build_dev.  Its device part (copies, gather,
     build; wall clock around a stream sync) and host part (writing the descriptors) are
     timed separately.  Both routes' resets are compared byte for byte first.
Each workload runs in a child process of its own under a time limit; the first failure ends
the run.
  python scripts/resetbench.py [--n 1048576 --rounds 5 --iters 20 --limit 300]"""
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

WORKLOADS = {"flood": dict(len_a=64, every=1), "sparse": dict(len_a=1500, every=100)}


def worker(args):
    import torch

    import rxg
    assert torch.cuda.is_available(), "resetbench needs a GPU"
    w = WORKLOADS[args.worker]
    n, L, nflows = args.n, w["len_a"], 10000
    slots = (L + 63) // 64
    dev = torch.device("cuda:0")
    eng = rxg.Engine(0)
    lib = rxg.load_library()
    ts = torch.cuda.Stream(dev)  # (not the null stream, which rxg takes as "the context's own")
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    # the flows whose TCB is missing get a reset; no listener (pass 2 finds nothing)
    tcb, live = rxg.synthetic_tcb_table(nflows)
    live[0] = 0
    live[1::w["every"]] = 0
    eng.tcb_load(tcb, live)
    sets = []
    for k in range(args.sets):
        # synthetic frames into torch's memory (the old route gathers from it with torch)
        p = rxg.SynthParams(77 + k, n, nflows, 0xC0A84E02, 80, 0, L, 0)
        nbytes = int(lib.rxg_synth_arena_bytes(C.byref(p)))
        d = dict(arena=torch.zeros(max(nbytes, n * slots * 64), dtype=torch.uint8, device=dev),
                 off64=torch.zeros(n, dtype=torch.int32, device=dev), len=torch.zeros(n, dtype=torch.int16, device=dev))
        used = C.c_uint64()
        rc = lib.rxg_synth_dev(eng.ctx, C.byref(p), d["arena"].data_ptr(), nbytes, d["off64"].data_ptr(),
                               d["len"].data_ptr(), None, C.byref(used), st)
        assert rc == 0, lib.rxg_last_error()
        recs = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
        eng.rx_burst_dev(d["arena"].data_ptr(), d["off64"].data_ptr(), d["len"].data_ptr(), n, recs.data_ptr(), rxg.REC8,
                         stream=st)
        eng.stream_sync(st)
        v = (recs.view(torch.int32)[0::2] >> 24) & 7
        count = int((v == rxg.V_RST_NOPCB).sum())
        assert int(((v == rxg.V_RST_NOPCB) | (v == rxg.V_RST_LISTEN_NONSYN)).sum()) == count
        # a fixed stride: the old route's 2-D view of the pool
        assert torch.equal(d["off64"], torch.arange(n, dtype=torch.int32, device=dev) * slots)
        sets.append(dict(d=d, recs=recs, count=count,
                         out=torch.zeros(max(count, 1) * 64, dtype=torch.uint8, device=dev),
                         idx=torch.zeros(max(count, 1), dtype=torch.int32, device=dev),
                         cnt=torch.zeros(1, dtype=torch.int64, device=dev),
                         out_b=torch.zeros(max(count, 1) * 64, dtype=torch.uint8, device=dev),
                         len_b=torch.zeros(max(count, 1), dtype=torch.int16, device=dev)))
    count = sets[0]["count"]
    assert count == n // w["every"] or abs(count - n / w["every"]) < 0.2 * n / w["every"], count

    def new_route(s):
        eng.tx_reset_dev(s["d"]["arena"].data_ptr(), s["d"]["len"].data_ptr(), n, s["recs"].data_ptr(), rxg.REC8,
                         s["out"].data_ptr(), s["idx"].data_ptr(), s["count"], s["cnt"].data_ptr(),
                         off64=s["d"]["off64"].data_ptr(), ip_id0=0, src_mac=rxg.REF_SRC_MAC, stream=st)

    def old_route(s, times=None):
        t0 = time.perf_counter()
        recs = s["recs"].view(torch.int32).cpu().numpy().reshape(n, 2)            # records to the host
        v = (recs[:, 0] >> 24) & 7
        sel = np.nonzero((v == rxg.V_RST_NOPCB) | (v == rxg.V_RST_LISTEN_NONSYN))[0]
        k = len(sel)
        d_sel = torch.from_numpy(sel).to(dev)
        pool = s["d"]["arena"][:n * slots * 64].view(n, slots * 64)
        lines = pool[d_sel, :64].cpu().numpy()                                     # offenders' first lines
        torch.cuda.current_stream().synchronize()
        t1 = time.perf_counter()
        flows = np.zeros(k, dtype=rxg.TX_FLOW_DTYPE)                              # one flow record per reset
        flows["dport"] = lines[:, 36:38].copy().view(">u2").ravel()               # becomes src_port
        flows["sport"] = lines[:, 34:36].copy().view(">u2").ravel()               # becomes dst_port
        flows["ipv4_dst"] = lines[:, 30:34].copy().view("<u4").ravel()            # src_addr, raw
        flows["ipv4_src"] = lines[:, 26:30].copy().view(">u4").ravel()            # dst_addr = htonl(this)
        flows["dst_mac"] = lines[:, 6:12]
        flows["src_mac"] = np.frombuffer(rxg.REF_SRC_MAC, np.uint8)
        segs = np.zeros(k, dtype=rxg.TX_SEG_DTYPE)
        segs["flow"] = np.arange(k)
        segs["seq"] = lines[:, 42:46].copy().view(">u4").ravel()
        segs["win_raw"], segs["tcp_flags"] = 12000, rxg.TCP_FLAG_RST
        segs["ip_id"] = np.arange(k) & 0xFFFF
        t2 = time.perf_counter()
        d_flows = torch.from_numpy(flows.view(np.uint8)).to(dev)
        d_segs = torch.from_numpy(segs.view(np.uint8)).to(dev)
        eng.tx_build_dev(d_segs.data_ptr(), 16, d_flows.data_ptr(), k, d_segs.data_ptr(), k, s["out_b"].data_ptr(),
                         s["len_b"].data_ptr(), None, 0, 1, None, stream=st)
        eng.stream_sync(st)
        t3 = time.perf_counter()
        if times is not None:
            times.append(((t1 - t0) + (t3 - t2), t2 - t1))

    for s in sets:  # both routes give the same resets
        new_route(s)
        old_route(s)
        torch.cuda.synchronize()
        assert int(s["cnt"][0]) == s["count"]
        assert torch.equal(s["out"], s["out_b"]), "rxg_tx_reset_dev and the rxg_tx_build_dev route differ"

    res, old_dev, old_host = [], [], []
    for _ in range(args.rounds):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
        for i, (a, e) in enumerate(evs):
            a.record()
            new_route(sets[i % len(sets)])
            e.record()
        torch.cuda.synchronize()
        res.append(float(np.median([a.elapsed_time(e) for a, e in evs])) * 1e3)
        tm = []
        for i in range(max(2, args.iters // 5)):
            old_route(sets[i % len(sets)], tm)
        old_dev.append(float(np.median([t[0] for t in tm])) * 1e6)
        old_host.append(float(np.median([t[1] for t in tm])) * 1e6)

    def row(name, us, **kw):
        med = float(np.median(us))
        print(json.dumps(dict(workload=args.worker, variant=name, n=n, frame_len=L, resets=count, us=round(med, 1),
                              rounds_us=[round(x, 1) for x in us],
                              spread_pct=round(100 * (max(us) - min(us)) / med, 2), **kw)), flush=True)
        return med
    alg = 2 * n * 8 + count * (64 + 64 + 4)
    a = row("a_tx_reset_dev", res, alg_bytes=alg, frac_8TBs=round(alg / (float(np.median(res)) * 1e-6) / 8e12, 4))
    bd = row("b_old_route_device_part", old_dev)
    bh = row("b_old_route_host_part", old_host)
    print(json.dumps(dict(workload=args.worker, ratio_old_device_part_to_a=round(bd / a, 1),
                          ratio_old_total_to_a=round((bd + bh) / a, 1))), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds each workload's process may take")
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    for name in ("flood", "sparse"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--n", str(args.n), "--sets", str(args.sets), "--rounds", str(args.rounds), "--iters", str(args.iters)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(f"resetbench: workload {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
