#!/usr/bin/env python3
"""Transmit segment build micro-benchmark: 2^20 segments x 1460 B of one contiguous send
buffer, 1 000 flows, frames at a fixed stride of 24 slots.  One run times, in interleaved
rounds on one stream,
  a  rxg_tx_build_dev (headers + payload + checksums in one pass)
  b  what the device could do before it: a device-to-device strided copy of the same payload
     bytes into pre-headered frames, then rxg_tx_cksum_dev over them; the copy is torch's
     copy_ of a strided uint8 view (b) or the runtime's hipMemcpy2DAsync (b2)
  c  rxg_tx_cksum_dev alone over the same frames
and, where the library has rxg_tx_build_opt_dev,
  a0 rxg_tx_build_opt_dev over the same descriptors (every reserved == 0: the option kernel
     doing the plain build's work)
  o  rxg_tx_build_opt_dev over 2^20 segments of --opt-len (1448) payload bytes that each carry
     the 12-byte timestamp block (one block in the table)
  bo (b) for those frames: the strided copy to frame byte 66 of frames that hold their headers
     and options already, then rxg_tx_cksum_dev
each over `--sets` rotating sets of buffers (a set is 3.1 GB at the default size, twelve times
the Infinity Cache, and a launch never meets the lines the launch before it left there).
Fractions of 8 TB/s are on the build's algorithmic bytes per segment: data_len + 32 + 64 *
ceil((54 + data_len) / 64) + 2; for (o) and (bo): data_len + 32 + 64 * ceil((66 + data_len) / 64)
+ 2, and 48 for the one block.  --variants a,o,.. times a subset (an older library: a, b, b2, c).
  python scripts/txbuildbench.py [--n 1048576 --len 1460 --rounds 5 --iters 20]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dpdk-tcpipstack_amd")]
import rxg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=1460)
    ap.add_argument("--flows", type=int, default=1000)
    ap.add_argument("--stride64", type=int, default=24)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--opt-len", type=int, default=1448)
    ap.add_argument("--variants", default="")
    args = ap.parse_args()
    n, L, stride = args.n, args.len, args.stride64
    LO, O = args.opt_len, 12  # the option legs: LO payload bytes after the 12-byte timestamp block
    assert 54 + O + LO <= stride * 64 and LO <= L
    assert torch.cuda.is_available(), "txbuildbench needs a GPU"
    assert 54 + L <= stride * 64
    dev = torch.device("cuda:0")
    eng = rxg.Engine(0)
    # torch's copies and rxg's launches on one stream of torch's (not the null stream, which rxg
    # takes as "the context's own")
    ts = torch.cuda.Stream(dev)
    torch.cuda.set_stream(ts)
    st = ts.cuda_stream
    assert st

    r = np.random.default_rng(3)
    flows = np.zeros(args.flows, dtype=rxg.TX_FLOW_DTYPE)
    flows["dport"], flows["sport"] = 80, 1024 + np.arange(args.flows)
    flows["ipv4_dst"] = rxg.ip_raw(10, 0, 0, 1)
    flows["ipv4_src"] = rxg.ip_host(172, 16, 0, 0) + np.arange(args.flows)
    flows["dst_mac"] = r.integers(0, 256, (args.flows, 6), dtype=np.uint8)
    flows["src_mac"] = np.frombuffer(rxg.REF_SRC_MAC, np.uint8)
    segs = np.zeros(n, dtype=rxg.TX_SEG_DTYPE)
    segs["src_off"] = np.arange(n, dtype=np.uint64) * L
    segs["flow"] = np.arange(n) % args.flows
    segs["seq"] = r.integers(0, 1 << 32, n, dtype=np.uint64)
    segs["ack"] = r.integers(0, 1 << 32, n, dtype=np.uint64)
    segs["data_len"], segs["win_raw"], segs["tcp_flags"] = L, 0xFFFF, rxg.TCP_FLAG_ACK
    segs["ip_id"] = np.arange(n) & 0xFFFF

    def dev_of(a):
        return torch.from_numpy(a.view(np.uint8).copy()).to(dev)
    d_flows, d_segs = dev_of(flows), dev_of(segs)
    has_opt = hasattr(rxg.load_library(), "rxg_tx_build_opt_dev")
    if has_opt:
        segs_o = segs.copy()
        segs_o["src_off"] = np.arange(n, dtype=np.uint64) * LO
        segs_o["data_len"], segs_o["reserved"] = LO, 1
        d_segs_o = dev_of(segs_o)
        d_opts = dev_of(np.array([rxg.tx_opt_timestamp(0x01020304, 0x05060708)], dtype=rxg.TX_OPT_DTYPE))
    d_stats = torch.zeros(2, dtype=torch.int64, device=dev)
    d_off = torch.arange(n, dtype=torch.int32, device=dev) * stride  # (c)'s offsets as a list
    pbytes = (n * L + 15) // 16 * 16
    sets = []
    for _ in range(args.sets):
        pay = torch.randint(0, 256, (pbytes,), dtype=torch.uint8, device=dev)
        sets.append(dict(pay=pay, built=torch.zeros(n * stride * 64, dtype=torch.uint8, device=dev),
                         pre=torch.zeros(n * stride * 64, dtype=torch.uint8, device=dev),
                         len=torch.zeros(n, dtype=torch.int16, device=dev)))
        if has_opt:
            sets[-1].update(pre_o=torch.zeros(n * stride * 64, dtype=torch.uint8, device=dev),
                            len_o=torch.zeros(n, dtype=torch.int16, device=dev))

    def build(s, frames):
        eng.tx_build_dev(s["pay"].data_ptr(), n * L, d_flows.data_ptr(), args.flows, d_segs.data_ptr(), n,
                         frames.data_ptr(), s["len"].data_ptr(), None, 0, stride, d_stats.data_ptr(), stream=st)

    def build_opt(s, frames, d_sg, lens, nbytes):
        eng.tx_build_opt_dev(s["pay"].data_ptr(), nbytes, d_flows.data_ptr(), args.flows, d_sg.data_ptr(), n,
                             frames.data_ptr(), lens.data_ptr(), d_opts.data_ptr(), 1, None, 0, stride,
                             d_stats.data_ptr(), stream=st)

    def copy_in_o(s):  # (bo): the payload bytes behind headers and options that are there already
        s["pre_o"].view(n, stride * 64)[:, 54 + O:54 + O + LO].copy_(s["pay"][:n * LO].view(n, LO))

    def cksum_o(s):
        eng.tx_cksum_dev(s["pre_o"].data_ptr(), d_off.data_ptr(), s["len_o"].data_ptr(), n, stream=st)

    def copy_in(s):  # the payload bytes into place, device to device
        s["pre"].view(n, stride * 64)[:, 54:54 + L].copy_(s["pay"][:n * L].view(n, L))

    hip = C.CDLL("libamdhip64.so")  # the runtime torch has loaded
    hip.hipMemcpy2DAsync.restype = C.c_int
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t,
                                     C.c_int, C.c_void_p]

    def copy2d_in(s):  # the same copy by the runtime: n rows of L bytes, pitch L -> pitch of a frame slot
        rc = hip.hipMemcpy2DAsync(s["pre"].data_ptr() + 54, stride * 64, s["pay"].data_ptr(), L, L, n,
                                  3, st)  # hipMemcpyDeviceToDevice
        assert rc == 0, f"hipMemcpy2DAsync: {rc}"

    def cksum(s):
        eng.tx_cksum_dev(s["pre"].data_ptr(), d_off.data_ptr(), s["len"].data_ptr(), n, stream=st)

    variants = {"a_tx_build": lambda s: build(s, s["built"]),
                "b_copy_then_cksum": lambda s: (copy_in(s), cksum(s)),
                "b2_memcpy2d_then_cksum": lambda s: (copy2d_in(s), cksum(s)),
                "c_cksum_alone": cksum}
    for s in sets:  # the pre-headered frames of (b) and (c): built once, then only rewritten
        build(s, s["pre"])
    torch.cuda.synchronize()
    assert d_stats.tolist() == [n * args.sets, 0], d_stats.tolist()
    # the three variants leave the same frames: (b) and (c) rewrite what the build wrote
    for s in sets:
        for f in variants.values():
            f(s)
    torch.cuda.synchronize()
    for s in sets:
        assert torch.equal(s["built"], s["pre"]), "copy + rxg_tx_cksum_dev and rxg_tx_build_dev differ"
    if has_opt:
        variants["a0_tx_build_opt_reserved0"] = lambda s: build_opt(s, s["built"], d_segs, s["len"], n * L)
        variants["o_tx_build_opt_ts12"] = lambda s: build_opt(s, s["built"], d_segs_o, s["len_o"], n * LO)
        variants["bo_copy_then_cksum_ts12"] = lambda s: (copy_in_o(s), cksum_o(s))
        # and so do the option legs: (a0) the plain build's frames, (o) and (bo) the same frames
        for s in sets:
            s["built"].zero_()
            variants["a0_tx_build_opt_reserved0"](s)
            torch.cuda.synchronize()
            assert torch.equal(s["built"], s["pre"]), "rxg_tx_build_opt_dev with reserved 0 and rxg_tx_build_dev differ"
            build_opt(s, s["pre_o"], d_segs_o, s["len_o"], n * LO)  # (bo)'s pre-headered frames
            s["built"].zero_()
            variants["o_tx_build_opt_ts12"](s)
            variants["bo_copy_then_cksum_ts12"](s)
            torch.cuda.synchronize()
            assert torch.equal(s["built"], s["pre_o"]), "copy + rxg_tx_cksum_dev and rxg_tx_build_opt_dev differ"
            assert int(s["len_o"][0]) == 54 + O + LO and int(s["built"].view(n, stride * 64)[n - 1, 46]) == 0x80
    only = [v for v in args.variants.split(",") if v]
    if only:
        variants = {k: f for k, f in variants.items() if k.split("_")[0] in only}
        assert variants, "no such variant"

    res = {k: [] for k in variants}
    for _ in range(args.rounds):
        for name, f in variants.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                   for _ in range(args.iters)]
            for i, (a, e) in enumerate(evs):
                a.record()
                f(sets[i % len(sets)])
                e.record()
            torch.cuda.synchronize()
            res[name].append(float(np.median([a.elapsed_time(e) for a, e in evs])))
    alg_plain = n * (L + 32 + 64 * ((54 + L + 63) // 64) + 2)
    alg_opt = n * (LO + 32 + 64 * ((54 + O + LO + 63) // 64) + 2) + 48
    for name, ms in res.items():
        med = float(np.median(ms))
        alg = alg_opt if name.endswith("_ts12") else alg_plain
        print(json.dumps({"variant": name, "n": n, "data_len": LO if name.endswith("_ts12") else L,
                          "us": round(med * 1e3, 1),
                          "rounds_us": [round(x * 1e3, 1) for x in ms],
                          "spread_pct": round(100 * (max(ms) - min(ms)) / med, 2),
                          "alg_bytes": alg, "frac_8TBs": round(alg / (med * 1e-3) / 8e12, 4)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
