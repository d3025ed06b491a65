#!/usr/bin/env python3
"""Received-option parse micro-benchmark (rxg_rx_opts_dev).  Three workloads of
2^20 segments each, built on the device at a fixed stride (rxg_tx_build_opt_dev) and classified
by a real burst with RXG_REC8 records (an empty table: every frame is RST_NOPCB, a candidate):
  ts     1 448 payload bytes behind the aligned timestamp block (O = 12)
  plain  the same without options
  small  64-byte frames (10 payload bytes, no options)
One run times, in interleaved rounds over `--sets` rotating sets of buffers on one stream,
  a  rxg_rx_opts_dev (one launch), fraction of 8 TB/s on its algorithmic bytes: n * 8 (records)
     + 2 n (len; fixed stride) + per candidate the 64-byte lines holding bytes 32 .. 54 + O
     inside the frame (128 for ts, 64 for plain and small) + 16 n written
  b  the route there was before it: the first 128 bytes of every frame (64 for `small`) and the
     records copied to the host (device part: wall clock around the copies), then
     rxg_rx_opt_parse per candidate on one core (host part).  The host part is timed through
     ctypes on the first `--host-frames` frames, less the same loop's time with len 0 (the
     call overhead), and scaled to n.  Both routes' records are compared whole first.
Each workload runs in a child process of its own under a time limit; the first failure ends
the run.
  python scripts/rxoptbench.py [--n 1048576 --rounds 5 --iters 20 --limit 300]"""
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

WORKLOADS = {"ts": dict(data=1448, opt=True, lines=2), "plain": dict(data=1448, opt=False, lines=1),
             "small": dict(data=10, opt=False, lines=1)}


def worker(args):
    import torch

    import rxg
    assert torch.cuda.is_available(), "rxoptbench needs a GPU"
    w = WORKLOADS[args.worker]
    n = args.n
    O = 12 if w["opt"] else 0
    flen = 54 + O + w["data"]
    stride64 = (flen + 63) // 64
    head = min(128, stride64 * 64)
    dev = torch.device("cuda:0")
    eng = rxg.Engine(0)
    lib = rxg.load_library()
    ts = torch.cuda.Stream(dev)  # (not the null stream, which rxg takes as "the context's own")
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    eng.tcb_load(*rxg_empty_table())

    def dev_of(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)

    flows = np.zeros(16, rxg.TX_FLOW_DTYPE)
    flows["dport"], flows["sport"] = 80, 40000 + np.arange(16)
    flows["ipv4_dst"], flows["ipv4_src"] = 0x024EA8C0, 0x0A000001 + np.arange(16)
    payload = dev_of(np.random.default_rng(1).integers(0, 256, 1 << 16, dtype=np.uint8))
    d_flows = dev_of(flows)
    sets = []
    for k in range(args.sets):
        rng = np.random.default_rng(100 + k)
        opts = np.concatenate([np.atleast_1d(rxg.tx_opt_timestamp(int(a), int(b)))
                               for a, b in rng.integers(0, 2**32, (64, 2))]).astype(rxg.TX_OPT_DTYPE)
        segs = np.zeros(n, rxg.TX_SEG_DTYPE)
        segs["flow"] = rng.integers(0, 16, n)
        segs["src_off"] = rng.integers(0, (1 << 16) - w["data"], n)
        segs["seq"], segs["ack"] = rng.integers(0, 2**32, n), rng.integers(0, 2**32, n)
        segs["data_len"], segs["tcp_flags"], segs["win_raw"] = w["data"], 0x10, 12000
        segs["reserved"] = rng.integers(1, 65, n) if w["opt"] else 0
        d_segs, d_opts = dev_of(segs), dev_of(opts)
        s = dict(arena=torch.zeros(n * stride64 * 64, dtype=torch.uint8, device=dev),
                 len=torch.zeros(n, dtype=torch.int16, device=dev), recs=torch.zeros(n * 8, dtype=torch.uint8, device=dev),
                 out=torch.zeros(n * 16, dtype=torch.uint8, device=dev))
        eng.tx_build_opt_dev(payload.data_ptr(), 1 << 16, d_flows.data_ptr(), 16, d_segs.data_ptr(), n, s["arena"].data_ptr(),
                             s["len"].data_ptr(), d_opts.data_ptr(), 64, None, 0, stride64, None, stream=st)
        eng.rx_bursts_strided_dev(s["arena"].data_ptr(), stride64, [(0, s["len"].data_ptr(), n, s["recs"].data_ptr())],
                                  rxg.REC8, stream=st)
        eng.stream_sync(st)
        assert int((s["len"].view(torch.int16) == flen).sum()) == n
        v = (s["recs"].view(torch.int32)[0::2] >> 24) & 7
        assert int((v == rxg.V_RST_NOPCB).sum()) == n
        s["want_ts"] = (opts["bytes"][:, 4:12].copy().view(">u4").reshape(-1, 2)[segs["reserved"] - 1] if w["opt"] else None)
        sets.append(s)

    def new_route(s):
        eng.rx_opts_dev(s["arena"].data_ptr(), s["len"].data_ptr(), n, s["recs"].data_ptr(), rxg.REC8, s["out"].data_ptr(),
                        off64=None, slot0=0, stride64=stride64, stream=st)

    def old_device_part(s):
        t0 = time.perf_counter()
        recs = s["recs"].view(torch.int32).cpu().numpy().reshape(n, 2)
        heads = s["arena"].view(n, stride64 * 64)[:, :head].contiguous().cpu().numpy()
        torch.cuda.current_stream().synchronize()
        return time.perf_counter() - t0, recs, heads

    def host_parse(heads, lens, m, out):
        parse, base = lib.rxg_rx_opt_parse, heads.ctypes.data
        t0 = time.perf_counter()
        for i in range(m):
            parse(base + i * head, lens[i], C.byref(out[i]))
        return time.perf_counter() - t0

    # both routes give the same records (and the timestamps that went in), on every frame of set 0
    lib.rxg_rx_opt_parse.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    for k, s in enumerate(sets):
        new_route(s)
        eng.stream_sync(st)
        got = s["out"].cpu().numpy().view(rxg.RX_OPT_DTYPE)
        assert (got["opt_len"] == O).all() and (got["flags"] == (rxg.O_PARSED | (rxg.O_TS if O else 0))).all()
        if O:
            assert np.array_equal(got["tsval"], s["want_ts"][:, 0]) and np.array_equal(got["tsecr"], s["want_ts"][:, 1])
        if k == 0:
            _, recs, heads = old_device_part(s)
            host_out = (rxg.RxOpt * n)()
            # (a frame longer than the copied head is parsed from its head: O <= 40 needs 94 bytes)
            host_parse(heads, [min(flen, head)] * n, n, host_out)
            host = np.frombuffer(host_out, dtype=rxg.RX_OPT_DTYPE)
            assert np.array_equal(host, got), "rxg_rx_opts_dev and the host route differ"

    res, old_dev, old_host = [], [], []
    m = min(n, args.host_frames)
    scratch = (rxg.RxOpt * m)()
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
            t, recs, heads = old_device_part(sets[i % len(sets)])
            tm.append(t)
        old_dev.append(float(np.median(tm)) * 1e6)
        real = host_parse(heads, [min(flen, head)] * m, m, scratch)
        call = host_parse(heads, [0] * m, m, scratch)
        old_host.append(max(real - call, 0.0) * n / m * 1e6)

    def row(name, us, **kw):
        med = float(np.median(us))
        print(json.dumps(dict(workload=args.worker, variant=name, n=n, frame_len=flen, us=round(med, 1),
                              rounds_us=[round(x, 1) for x in us],
                              spread_pct=round(100 * (max(us) - min(us)) / med, 2), **kw)), flush=True)
        return med
    alg = n * 8 + 2 * n + n * 64 * w["lines"] + 16 * n
    a = row("a_rx_opts_dev", res, alg_bytes=alg, frac_8TBs=round(alg / (float(np.median(res)) * 1e-6) / 8e12, 4))
    bd = row("b_old_route_device_part", old_dev)
    bh = row("b_old_route_host_part", old_host, host_frames=m)
    print(json.dumps(dict(workload=args.worker, ratio_old_device_part_to_a=round(bd / a, 1),
                          ratio_old_total_to_a=round((bd + bh) / a, 1))), flush=True)
    eng.close()


def rxg_empty_table():
    import rxg
    return np.zeros(0, dtype=rxg.TCB_DTYPE), np.zeros(0, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=1 << 17)
    ap.add_argument("--limit", type=int, default=300, help="seconds each workload's process may take")
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    for name in ("ts", "plain", "small"):
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--n", str(args.n), "--sets", str(args.sets), "--rounds", str(args.rounds), "--iters", str(args.iters),
               "--host-frames", str(args.host_frames)]
        rc = subprocess.run(cmd).returncode
        if rc:
            sys.exit(f"rxoptbench: workload {name} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
