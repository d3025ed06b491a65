"""CPU: the host side of the option build -- rxg_tx_build_opt_dev and its helpers at the C
boundary (declared, exported, layouts by a compiled probe, argument errors without a context),
the three block helpers against bytes written out here, rxg_tx_plan_opt against rxg_tx_plan,
both stand-alone under ASan/UBSan (tests/txopt_check.cpp), and the model the GPU tests compare
with (tests/txbuild_opt_ref.py) pinned against a hand-built sendack frame and the rx oracle."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle
import rxg
import txbuild_opt_ref as oref
import txbuild_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc")
EINVAL, ENOSPC = 22, 28
SYN, FIN, PSH, ACK = 0x02, 0x01, 0x08, 0x10
NAMES = ("rxg_tx_build_opt_dev", "rxg_tx_opt_set", "rxg_tx_opt_timestamp", "rxg_tx_opt_ref_ack", "rxg_tx_plan_opt")

# the 20 option bytes of sendtcpack (tcp_out.c:255-262): timestamp 203032 / 0 as the host holds
# them, MSS htons(1300), window scale 7, three bytes of pad
REF_ACK = bytes([8, 10, 0x18, 0x19, 0x03, 0x00, 0, 0, 0, 0, 2, 4, 0x05, 0x14, 3, 3, 7, 0, 0, 0])


def test_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "rxg.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
    out = subprocess.run(["nm", "-D", "--defined-only", rxg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert set(NAMES) <= set(re.findall(r"\bT (\w+)", out))
    assert rxg.load_library().rxg_abi_version() == 2


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "rxg.h"
#define S(t) printf("sizeof " #t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
    S(rxg_tx_opt); O(rxg_tx_opt, len); O(rxg_tx_opt, reserved0); O(rxg_tx_opt, bytes); O(rxg_tx_opt, reserved1);
    S(rxg_dev_tx_build_opt); O(rxg_dev_tx_build_opt, b); O(rxg_dev_tx_build_opt, opts);
    O(rxg_dev_tx_build_opt, nopts); O(rxg_dev_tx_build_opt, pad);
    S(rxg_tx_seg); O(rxg_tx_seg, reserved); S(rxg_tx_flow); O(rxg_tx_flow, reserved); S(rxg_dev_tx_build);
    return 0;
}
"""


def test_struct_layouts_by_c_probe(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", INC, str(tmp_path / "probe.c"), "-o",
                    str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    assert got["sizeof rxg_tx_opt"] == 48 and got["rxg_tx_opt.bytes"] == 6
    assert got["rxg_tx_opt.len"] == 0 and got["rxg_tx_opt.reserved0"] == 1 and got["rxg_tx_opt.reserved1"] == 46
    # no existing layout moved
    assert got["sizeof rxg_tx_seg"] == 32 and got["rxg_tx_seg.reserved"] == 28
    assert got["sizeof rxg_tx_flow"] == 32 and got["rxg_tx_flow.reserved"] == 24 and got["sizeof rxg_dev_tx_build"] == 80
    assert got["rxg_dev_tx_build_opt.b"] == 0 and got["rxg_dev_tx_build_opt.opts"] == 80
    for name, dt, cs in (("rxg_tx_opt", rxg.TX_OPT_DTYPE, rxg.TxOpt), ("rxg_dev_tx_build_opt", None, rxg.DevTxBuildOpt)):
        assert got["sizeof " + name] == C.sizeof(cs)
        for f, *_ in cs._fields_:
            assert got[f"{name}.{f}"] == getattr(cs, f).offset, (name, f)
            if dt is not None:
                assert got[f"{name}.{f}"] == dt.fields[f][1], (name, f)
        if dt is not None:
            assert dt.itemsize == C.sizeof(cs)


# ------------------------------------------------------------------- the helpers ---
def test_opt_set_pads_and_zeroes():
    lib = rxg.load_library()
    for n in range(41):
        data = bytes(range(1, n + 1))
        o = np.full(1, 0xEE, dtype=np.uint8).repeat(48).view(rxg.TX_OPT_DTYPE)
        raw = np.frombuffer(data, np.uint8)
        rc = lib.rxg_tx_opt_set(o.ctypes.data, raw.ctypes.data if n else None, n)
        assert rc == (n + 3) // 4 * 4 == int(o[0]["len"])
        assert o.tobytes() == bytes([rc]) + bytes(5) + data + bytes(40 - n) + bytes(2), n
        assert rxg.tx_opt_set(data).tobytes() == o.tobytes()
    o = np.zeros(1, dtype=rxg.TX_OPT_DTYPE)
    raw = np.zeros(64, np.uint8)
    assert lib.rxg_tx_opt_set(o.ctypes.data, raw.ctypes.data, 41) == -EINVAL
    assert lib.rxg_tx_opt_set(None, raw.ctypes.data, 4) == -EINVAL
    assert lib.rxg_tx_opt_set(o.ctypes.data, None, 4) == -EINVAL
    with pytest.raises(rxg.RxgError):
        rxg.tx_opt_set(bytes(41))


def test_opt_timestamp_bytes():
    o = rxg.tx_opt_timestamp(0x01020304, 0xA0B0C0D0)
    assert int(o["len"]) == 12
    assert o["bytes"].tobytes() == bytes([1, 1, 8, 10, 1, 2, 3, 4, 0xA0, 0xB0, 0xC0, 0xD0]) + bytes(28)
    assert not o["reserved0"].any() and not o["reserved1"].any()
    assert rxg.load_library().rxg_tx_opt_timestamp(None, 1, 2) == -EINVAL


def test_opt_ref_ack_bytes():
    o = rxg.tx_opt_ref_ack()
    assert int(o["len"]) == 20 == len(REF_ACK)
    assert o["bytes"].tobytes() == REF_ACK + bytes(20)
    assert REF_ACK[2:6] == struct.pack("<I", 203032) and REF_ACK[12:14] == struct.pack("!H", 1300)
    assert not o["reserved0"].any() and not o["reserved1"].any()
    assert rxg.load_library().rxg_tx_opt_ref_ack(None) == -EINVAL


# ------------------------------------------------------------------- the planner ---
MSS = 1460
SIZES = [0, 1, MSS - 13, MSS - 12, MSS - 11, MSS, 3 * MSS + 7]
FLAGS = [0, SYN, FIN, SYN | FIN, ACK | PSH]


def _sends():
    return [(k % 5, 0xFFFFF000 + 97 * k, 1000 + k, 31 * k, b, f, 0xFFFF, 0xFFFE)
            for k, (b, f) in enumerate((b, f) for b in SIZES for f in FLAGS)]


def _send_array(rows):
    a = np.zeros(len(rows), dtype=rxg.TX_SEND_DTYPE)
    for i, r in enumerate(rows):
        for k, v in zip(("flow", "next_seq", "ack", "src_off", "bytes", "tcp_flags", "win_raw", "ip_id0"), r):
            a[i][k] = v
    return a


def test_plan_opt_without_send_opt_is_plan():
    lib = rxg.load_library()
    sends = _send_array(_sends())
    want, wnext = rxg.tx_plan(sends, MSS)
    cap = len(want)
    out = np.full(cap + 2, 0xEE, dtype=np.uint8).repeat(32).view(rxg.TX_SEG_DTYPE)
    nxt = np.zeros(len(sends), np.uint32)
    opts = oref.make_opts()
    assert lib.rxg_tx_plan_opt(sends.ctypes.data, len(sends), MSS, None, opts.ctypes.data, len(opts), out.ctypes.data,
                               cap, nxt.ctypes.data) == cap
    assert out[:cap].tobytes() == want.tobytes() and np.array_equal(nxt, wnext)
    assert (out[cap:].view(np.uint8) == 0xEE).all()
    segs, nxt2 = rxg.tx_plan_opt(sends, MSS, None, opts)
    assert segs.tobytes() == want.tobytes() and np.array_equal(nxt2, wnext)
    # send_opt all zero: the same again
    segs, nxt2 = rxg.tx_plan_opt(sends, MSS, np.zeros(len(sends), np.uint32), opts)
    assert segs.tobytes() == want.tobytes() and np.array_equal(nxt2, wnext)


def test_plan_opt_cuts_at_mss_less_the_block():
    sends = _send_array(_sends())
    opts = np.array([rxg.tx_opt_timestamp(7, 9), rxg.tx_opt_ref_ack()], dtype=rxg.TX_OPT_DTYPE)
    send_opt = (np.arange(len(sends)) % 3).astype(np.uint32)  # none, the 12-byte block, the 20-byte block
    segs, nxt = rxg.tx_plan_opt(sends, MSS, send_opt, opts)
    at = 0
    for j in range(len(sends)):
        O = (0, 12, 20)[int(send_opt[j])]
        want, wnext = rxg.tx_plan(sends[j:j + 1], MSS - O)  # cut at mss - O ...
        mine = segs[at:at + len(want)]
        assert (mine["reserved"] == send_opt[j]).all()
        assert (mine["data_len"] <= MSS - O).all()
        want["reserved"] = send_opt[j]                   # ... and nothing else differs
        assert mine.tobytes() == want.tobytes(), j
        _, plain_next = rxg.tx_plan(sends[j:j + 1], MSS)
        assert int(nxt[j]) == int(wnext[0]) == int(plain_next[0])  # the same bytes, the same next_seq
        at += len(want)
    assert at == len(segs)
    one, _ = rxg.tx_plan_opt([(0, 1, 2, 0, 3 * (MSS - 12), ACK, 1, 1)], MSS, [1], opts)
    assert list(one["data_len"]) == [MSS - 12] * 3 and list(one["src_off"]) == [0, MSS - 12, 2 * (MSS - 12)]


def test_plan_opt_errors():
    lib = rxg.load_library()
    sends = _send_array([(0, 1, 2, 0, 5000, ACK, 1, 1), (1, 1, 2, 0, 100, ACK, 1, 1)])
    opts = oref.make_opts([12, 44, 6, 40])
    out = np.full(64, 0xEE, dtype=np.uint8).repeat(32).view(rxg.TX_SEG_DTYPE)

    def call(send_opt, mss=MSS, opts_ptr=opts.ctypes.data, nopts=len(opts), cap=64):
        so = np.array(send_opt, np.uint32)
        return lib.rxg_tx_plan_opt(sends.ctypes.data, 2, mss, so.ctypes.data, opts_ptr, nopts, out.ctypes.data, cap, None)
    assert call([1, 0]) == 5 and (out[:5]["reserved"] == [1, 1, 1, 1, 0]).all()
    out.view(np.uint8)[:] = 0xEE
    for so, kw in [([0, 5], {}), ([0, 2], {}), ([0, 3], {}), ([1, 0], dict(nopts=0)), ([0, 1], dict(mss=12)),
                   ([0, 4], dict(mss=40)), ([0, 1], dict(opts_ptr=None)), ([0, 0], dict(mss=0)),
                   ([0, 0], dict(mss=rxg.TX_MAX_DATA + 1))]:
        assert call(so, **kw) == -EINVAL, (so, kw)
        assert (out.view(np.uint8) == 0xEE).all(), (so, kw)  # the second send's error: nothing of the first written
    assert call([0, 4], mss=1000) == 5 + 1 and int(out[5]["data_len"]) == 100  # mss > O suffices
    out.view(np.uint8)[:] = 0xEE
    assert call([1, 0], cap=4) == -ENOSPC
    assert (out[4:].view(np.uint8) == 0xEE).all()
    with pytest.raises(rxg.RxgError):
        rxg.tx_plan_opt(sends, MSS, [0, 5], opts)


def test_helpers_and_planner_standalone_sanitized(tmp_path):
    exe = tmp_path / "txopt_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", INC, os.path.join(ROOT, "tests", "txopt_check.cpp"),
                    os.path.join(CSRC, "rxg_txopt.cpp"), os.path.join(CSRC, "rxg_txplan.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "txopt ok" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


def test_null_arguments():
    lib = rxg.load_library()
    b = rxg.DevTxBuildOpt()
    assert lib.rxg_tx_build_opt_dev(None, C.byref(b), None) == -EINVAL
    assert b"rxg_tx_build_opt_dev" in lib.rxg_last_error() and b"NULL" in lib.rxg_last_error()


# --------------------------------------------------------- the model, pinned ---
def rfc1071(data: bytes) -> int:
    if len(data) % 2:
        data += b"\0"
    s = sum(struct.unpack("!%dH" % (len(data) // 2), data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def _one_flow():
    flows = np.zeros(1, dtype=rxg.TX_FLOW_DTYPE)
    flows[0]["dport"], flows[0]["sport"] = 80, 51234
    flows[0]["ipv4_dst"] = rxg.ip_raw(10, 0, 0, 1)
    flows[0]["ipv4_src"] = rxg.ip_host(192, 168, 7, 9)
    flows[0]["dst_mac"] = [2, 4, 6, 8, 10, 12]
    flows[0]["src_mac"] = np.frombuffer(rxg.REF_SRC_MAC, np.uint8)
    return flows


def _peer_tcb(flows):
    tcb = np.zeros(len(flows), dtype=rxg.TCB_DTYPE)
    tcb["dport"], tcb["sport"] = flows["sport"], flows["dport"]
    tcb["ipv4_dst"] = flows["ipv4_src"].byteswap()
    tcb["ipv4_src"] = flows["ipv4_dst"].byteswap()
    tcb["state"] = rxg.TCP_ESTABLISHED
    return tcb


def test_model_sendack_frame_by_hand_and_through_the_rx_oracle():
    """sendack: rxg_tx_opt_ref_ack's block, flags ACK, rx_win 12000 raw, no data
    (tcp_out.c:251-289).  The frame put together field by field in wire order, and the model's
    frame through the receive oracle: both checksums 0, datalen 0, data_off 0xA0."""
    flows = _one_flow()
    opts = np.array([rxg.tx_opt_ref_ack()], dtype=rxg.TX_OPT_DTYPE)
    segs = np.zeros(1, dtype=rxg.TX_SEG_DTYPE)
    segs[0] = (0, 0, 0x01020304, 0xA0B0C0D0, 0, 12000, 0x0102, ACK, 0, 1)
    pool, lens, stats = oref.build(np.zeros(16, np.uint8), flows, segs, opts, [0], 2, fill=0xA5)
    assert list(stats) == [1, 0] and int(lens[0]) == 74
    ip0 = struct.pack("!BBH", 0x45, 0, 60) + struct.pack("<H", 0x0102) + struct.pack("!HBB", 0, 127, 6)
    addrs = bytes([10, 0, 0, 1, 192, 168, 7, 9])
    ip = ip0 + struct.pack("!H", rfc1071(ip0 + b"\0\0" + addrs)) + addrs
    tcp0 = struct.pack("!HHIIBB", 80, 51234, 0x01020304, 0xA0B0C0D0, 0xA0, ACK) + struct.pack("<H", 12000)
    ck = rfc1071(addrs + struct.pack("!BBH", 0, 6, 40) + tcp0 + b"\0\0\0\0" + REF_ACK)
    want = bytes([2, 4, 6, 8, 10, 12]) + rxg.REF_SRC_MAC + b"\x08\x00" + ip + tcp0 + struct.pack("!HH", ck, 0) + REF_ACK
    assert len(want) == 74 and pool[:74].tobytes() == want
    assert not pool[74:128].any() and (pool[128:] == 0xA5).all()
    recs, _ = oracle.rx_batch(pool, np.array([0], np.uint32), lens, _peer_tcb(flows), np.ones(1, np.uint8))
    assert int(recs["c"]["ip_cksum"][0]) == 0 and int(recs["c"]["tcp_cksum"][0]) == 0
    assert int(recs["c"]["verdict"][0]) == rxg.V_DISPATCH and int(recs["c"]["datalen"][0]) == 0
    assert int(recs["data_off"][0]) == 0xA0


def test_model_frames_of_every_block_verify_through_the_rx_oracle():
    flows = ref.make_flows()
    opts = oref.make_opts()
    r = np.random.default_rng(3)
    cases = [(k, L) for k in range(len(opts) + 1) for L in oref.payload_lengths(int(opts[k - 1]["len"]) if k else 0)]
    payload = r.integers(0, 256, 8192, dtype=np.uint8)
    dl = np.array([L for _, L in cases])
    segs = ref.make_segs(dl, r.integers(0, 8192 - 2731, len(cases)), len(flows), seed=4)
    segs["reserved"] = [k for k, _ in cases]
    ol = oref.opt_len(segs, opts)
    assert sorted(set(ol.tolist())) == oref.OPT_LENS
    off, nslots = oref.packed_offsets(dl, ol)
    pool, flen, stats = oref.build(payload, flows, segs, opts, off, nslots)
    assert list(stats) == [len(cases), 0] and np.array_equal(flen, oref.frame_lens(dl, ol))
    # with reserved 0 everywhere the model is txbuild_ref's
    plain = segs.copy()
    plain["reserved"] = 0
    off0, nslots0 = ref.packed_offsets(dl)
    a = oref.build(payload, flows, plain, opts, off0, nslots0, fill=0xA5)
    b = ref.build(payload, flows, plain, off0, nslots0, fill=0xA5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    recs, _ = oracle.rx_batch(pool, off, flen, _peer_tcb(flows), np.ones(len(flows), np.uint8))
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all() and (recs["c"]["tcb_idx"] == segs["flow"]).all()
    assert (recs["c"]["datalen"] == dl).all()
    assert np.array_equal(recs["data_off"], ((5 + ol // 4) << 4).astype(np.uint8))
    for i, (k, L) in enumerate(cases):  # the option bytes and the payload stand where rxg.h says
        a0, O, o = int(off[i]) * 64 + 54, int(ol[i]), int(segs["src_off"][i])
        if k:
            assert np.array_equal(pool[a0:a0 + O], opts[k - 1]["bytes"][:O])
        assert np.array_equal(pool[a0 + O:a0 + O + L], payload[o:o + L])
