"""CPU: the transmit segment build's host side -- rxg_tx_build_dev / rxg_tx_plan at the C
boundary (declared, exported, struct layouts, argument errors without a context), the planner
against a restatement of tcp_out.c:176-185, the planner stand-alone under ASan/UBSan, and the
reference model the GPU tests compare with (tests/txbuild_ref.py) pinned against frames put
together by hand and against the receive oracle."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle
import rxg
import txbuild_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
EINVAL, ENOSPC = 22, 28
SYN, FIN, PSH, ACK = 0x02, 0x01, 0x08, 0x10


# ------------------------------------------------------------- 1. exports, arguments ---
def test_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "rxg.h")).read(), flags=re.S)
    for name in ("rxg_tx_build_dev", "rxg_tx_plan"):
        assert re.search(r"\b%s\s*\(" % name, src), name
    out = subprocess.run(["nm", "-D", "--defined-only", rxg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (\w+)", out))
    assert {"rxg_tx_build_dev", "rxg_tx_plan"} <= exported
    assert all(s.startswith("rxg_") for s in exported), sorted(s for s in exported if not s.startswith("rxg_"))


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "rxg.h"
#define S(t) printf("sizeof " #t " %zu\n", sizeof(t))
#define O(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void)
{
    S(rxg_tx_flow); O(rxg_tx_flow, dport); O(rxg_tx_flow, sport); O(rxg_tx_flow, ipv4_dst); O(rxg_tx_flow, ipv4_src);
    O(rxg_tx_flow, dst_mac); O(rxg_tx_flow, src_mac); O(rxg_tx_flow, reserved);
    S(rxg_tx_seg); O(rxg_tx_seg, src_off); O(rxg_tx_seg, flow); O(rxg_tx_seg, seq); O(rxg_tx_seg, ack);
    O(rxg_tx_seg, data_len); O(rxg_tx_seg, win_raw); O(rxg_tx_seg, ip_id); O(rxg_tx_seg, tcp_flags);
    O(rxg_tx_seg, pad); O(rxg_tx_seg, reserved);
    S(rxg_dev_tx_build); O(rxg_dev_tx_build, payload); O(rxg_dev_tx_build, payload_bytes);
    O(rxg_dev_tx_build, flows); O(rxg_dev_tx_build, nflows); O(rxg_dev_tx_build, n); O(rxg_dev_tx_build, segs);
    O(rxg_dev_tx_build, frames); O(rxg_dev_tx_build, off64); O(rxg_dev_tx_build, slot0);
    O(rxg_dev_tx_build, stride64); O(rxg_dev_tx_build, len); O(rxg_dev_tx_build, stats);
    S(rxg_tx_send); O(rxg_tx_send, flow); O(rxg_tx_send, next_seq); O(rxg_tx_send, ack); O(rxg_tx_send, src_off);
    O(rxg_tx_send, bytes); O(rxg_tx_send, tcp_flags); O(rxg_tx_send, win_raw); O(rxg_tx_send, ip_id0);
    printf("RXG_TX_MAX_DATA %u\n", RXG_TX_MAX_DATA);
    { const unsigned char m[6] = RXG_REF_SRC_MAC; printf("mac %02x%02x%02x%02x%02x%02x\n", m[0], m[1], m[2], m[3], m[4], m[5]); }
    return 0;
}
"""


def test_struct_layouts_by_c_probe(tmp_path):
    d = tmp_path / "txbuild_probe"
    d.mkdir()
    (d / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", INC, str(d / "probe.c"), "-o",
                    str(d / "probe")], check=True)
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.strip().splitlines())
    assert got["sizeof rxg_tx_flow"] == "32" and got["sizeof rxg_tx_seg"] == "32"
    assert int(got["sizeof rxg_dev_tx_build"]) == 80 and int(got["sizeof rxg_tx_send"]) % 8 == 0
    for struct_name, dt, cs in (("rxg_tx_flow", rxg.TX_FLOW_DTYPE, rxg.TxFlow), ("rxg_tx_seg", rxg.TX_SEG_DTYPE, rxg.TxSeg),
                                ("rxg_tx_send", rxg.TX_SEND_DTYPE, rxg.TxSend), ("rxg_dev_tx_build", None, rxg.DevTxBuild)):
        assert int(got["sizeof " + struct_name]) == C.sizeof(cs)
        for f, *_ in cs._fields_:
            key = f"{struct_name}.{f}"
            if key in got:
                assert int(got[key]) == getattr(cs, f).offset, key
                if dt is not None:
                    assert int(got[key]) == dt.fields[f][1], key
        if dt is not None:
            assert dt.itemsize == C.sizeof(cs)
    assert int(got["RXG_TX_MAX_DATA"]) == rxg.TX_MAX_DATA == 65535 - 54
    assert got["mac"] == rxg.REF_SRC_MAC.hex()


def test_null_arguments_and_abi():
    lib = rxg.load_library()
    assert lib.rxg_abi_version() == 2
    b = rxg.DevTxBuild()
    assert lib.rxg_tx_build_dev(None, C.byref(b), None) == -EINVAL
    assert b"NULL" in lib.rxg_last_error()
    s = np.zeros(1, dtype=rxg.TX_SEND_DTYPE)
    o = np.zeros(1, dtype=rxg.TX_SEG_DTYPE)
    assert lib.rxg_tx_plan(s.ctypes.data, 1, 0, o.ctypes.data, 1, None) == -EINVAL
    assert lib.rxg_tx_plan(s.ctypes.data, 1, rxg.TX_MAX_DATA + 1, o.ctypes.data, 1, None) == -EINVAL
    assert lib.rxg_tx_plan(None, 1, 1460, o.ctypes.data, 1, None) == -EINVAL
    assert lib.rxg_tx_plan(s.ctypes.data, 1, rxg.TX_MAX_DATA, o.ctypes.data, 1, None) == 1


# ------------------------------------------------------------------- 2. the planner ---
def plan_py(send, mss):
    """tcp_out.c:176-185, one sendtcpdata per segment."""
    flow, seq, ack, off, nbytes, flags, win, ipid = send
    nseg = max(1, -(-nbytes // mss))
    out = []
    for q in range(nseg):
        n = min(mss, nbytes - q * mss)
        fl = flags & ~(SYN | FIN | PSH) | (flags & SYN if q == 0 else 0) | (flags & (FIN | PSH) if q == nseg - 1 else 0)
        out.append((off + q * mss, flow, seq, ack, n, win, (ipid + q) & 0xFFFF, fl))
        seq = (seq + n + bool(fl & SYN) + bool(fl & FIN)) & 0xFFFFFFFF
    return out, seq


MSS = 1460
SIZES = [0, 1, MSS - 1, MSS, MSS + 1, 3 * MSS, 3 * MSS + 7]
FLAGS = [0, SYN, FIN, SYN | FIN, ACK | PSH]


def _sends():
    return [(k % 5, 0xFFFFF000 + 97 * k, 1000 + k, 31 * k, b, f, 0xFFFF, 0xFFFE)
            for k, (b, f) in enumerate((b, f) for b in SIZES for f in FLAGS)]


def _rows(segs):
    return [tuple(int(s[k]) for k in ("src_off", "flow", "seq", "ack", "data_len", "win_raw", "ip_id", "tcp_flags"))
            for s in segs]


@pytest.mark.parametrize("nbytes", SIZES)
@pytest.mark.parametrize("flags", FLAGS)
def test_plan_one_send(nbytes, flags):
    send = (2, 0xFFFFFF00, 5, 123, nbytes, flags, 0xFFFF, 0xFFFE)
    want, want_next = plan_py(send, MSS)
    segs, nxt = rxg.tx_plan([send], MSS)
    assert _rows(segs) == want and int(nxt[0]) == want_next
    assert (segs["pad"] == 0).all() and (segs["reserved"] == 0).all()
    if len(want) > 1:
        assert [r[6] for r in want[:3]] == [0xFFFE, 0xFFFF, 0][:len(want)]  # ip_id wraps
        assert not any(r[7] & SYN for r in want[1:]) and not any(r[7] & (FIN | PSH) for r in want[:-1])


def test_plan_batch_and_capacity():
    lib = rxg.load_library()
    sends = _sends()
    want = [r for s in sends for r in plan_py(s, MSS)[0]]
    segs, nxt = rxg.tx_plan(sends, MSS)
    assert _rows(segs) == want
    assert [int(x) for x in nxt] == [plan_py(s, MSS)[1] for s in sends]
    # cap one short: -ENOSPC and nothing written at or past cap
    arr = np.zeros(len(sends), dtype=rxg.TX_SEND_DTYPE)
    for i, r in enumerate(sends):
        for k, v in zip(("flow", "next_seq", "ack", "src_off", "bytes", "tcp_flags", "win_raw", "ip_id0"), r):
            arr[i][k] = v
    cap = len(want)
    out = np.full(cap + 4, 0xEE, dtype=np.uint8).repeat(32).view(rxg.TX_SEG_DTYPE)
    assert lib.rxg_tx_plan(arr.ctypes.data, len(arr), MSS, out.ctypes.data, cap, None) == cap
    assert (out[cap:].view(np.uint8) == 0xEE).all() and _rows(out[:cap]) == want
    out = np.full(cap + 4, 0xEE, dtype=np.uint8).repeat(32).view(rxg.TX_SEG_DTYPE)
    assert lib.rxg_tx_plan(arr.ctypes.data, len(arr), MSS, out.ctypes.data, cap - 1, None) == -ENOSPC
    assert (out[cap - 1:].view(np.uint8) == 0xEE).all()


# ------------------------------------------------ 3. the planner under ASan / UBSan ---
def test_plan_standalone_sanitized(tmp_path):
    exe = tmp_path / "txplan_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", INC, os.path.join(ROOT, "tests", "txplan_check.cpp"),
                    os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc", "rxg_txplan.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "txplan ok" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


# ------------------------------------------------------- the reference model, pinned ---
def rfc1071(data: bytes) -> int:
    """RFC 1071: the 16-bit one's complement of the one's complement sum of the big-endian
    16-bit words, an odd last byte padded with zero."""
    if len(data) % 2:
        data += b"\0"
    s = sum(struct.unpack("!%dH" % (len(data) // 2), data))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def hand_frame(dst_mac, src_mac, src_ip, dst_ip, sport, dport, seq, ack, flags, win_le, ipid_le, payload):
    """A frame put together field by field in wire order with struct.pack."""
    ip0 = struct.pack("!BBH", 0x45, 0, 40 + len(payload)) + struct.pack("<H", ipid_le) + \
        struct.pack("!HBB", 0, 127, 6)
    addrs = bytes(src_ip) + bytes(dst_ip)
    ip = ip0 + struct.pack("!H", rfc1071(ip0 + b"\0\0" + addrs)) + addrs
    tcp0 = struct.pack("!HHIIBB", sport, dport, seq, ack, 0x50, flags) + struct.pack("<H", win_le)
    pseudo = addrs + struct.pack("!BBH", 0, 6, 20 + len(payload))
    ck = rfc1071(pseudo + tcp0 + b"\0\0\0\0" + payload)
    return bytes(dst_mac) + bytes(src_mac) + b"\x08\x00" + ip + tcp0 + struct.pack("!HH", ck, 0) + payload


HAND = [  # (payload, flags, seq, ack, win, ip_id)
    (b"", ACK, 1, 2, 0xFFFF, 0),
    (b"hello, world", ACK | PSH, 0x01020304, 0xA0B0C0D0, 0x1234, 0xFFFE),
    (bytes(range(251)) * 3, FIN | ACK, 0xFFFFFFFF, 0, 0x00FF, 0x0100),
]


def test_model_equals_hand_built_frames():
    flows = np.zeros(1, dtype=rxg.TX_FLOW_DTYPE)
    flows[0]["dport"], flows[0]["sport"] = 80, 51234
    flows[0]["ipv4_dst"] = rxg.ip_raw(10, 0, 0, 1)        # our address, as stored in the TCB
    flows[0]["ipv4_src"] = rxg.ip_host(192, 168, 7, 9)    # the peer's, host order
    flows[0]["dst_mac"] = [2, 4, 6, 8, 10, 12]
    flows[0]["src_mac"] = np.frombuffer(rxg.REF_SRC_MAC, np.uint8)
    payload = np.frombuffer(b"".join(h[0] for h in HAND) + bytes(16), np.uint8)
    segs = np.zeros(len(HAND), dtype=rxg.TX_SEG_DTYPE)
    o = 0
    for i, (p, fl, seq, ack, win, ipid) in enumerate(HAND):
        segs[i] = (o, 0, seq, ack, len(p), win, ipid, fl, 0, 0)
        o += len(p)
    off, nslots = ref.packed_offsets(segs["data_len"])
    pool, lens, stats = ref.build(payload, flows, segs, off, nslots, fill=0xA5)
    assert list(stats) == [len(HAND), 0]
    for i, (p, fl, seq, ack, win, ipid) in enumerate(HAND):
        want = hand_frame([2, 4, 6, 8, 10, 12], rxg.REF_SRC_MAC, [10, 0, 0, 1], [192, 168, 7, 9], 80, 51234, seq, ack,
                          fl, win, ipid, p)
        a = int(off[i]) * 64
        assert int(lens[i]) == len(want) == 54 + len(p)
        assert pool[a:a + len(want)].tobytes() == want, i
        end = (len(want) + 63) // 64 * 64
        assert not pool[a + len(want):a + end].any()


def test_model_frames_verify_through_the_rx_oracle():
    flows = ref.make_flows()
    r = np.random.default_rng(3)
    lens = np.array(ref.LENGTHS)
    payload = r.integers(0, 256, 70000, dtype=np.uint8)
    segs = ref.make_segs(lens, r.integers(0, 70000 - 65481, len(lens)), len(flows), seed=4)
    off, nslots = ref.packed_offsets(lens)
    pool, flen, _ = ref.build(payload, flows, segs, off, nslots)
    tcb = np.zeros(len(flows), dtype=rxg.TCB_DTYPE)
    # the peer's TCB for our segment: its local port is our dst_port, its address our dst_addr
    tcb["dport"], tcb["sport"] = flows["sport"], flows["dport"]
    tcb["ipv4_dst"] = flows["ipv4_src"].byteswap()
    tcb["ipv4_src"] = flows["ipv4_dst"].byteswap()
    tcb["state"] = rxg.TCP_ESTABLISHED
    recs, _ = oracle.rx_batch(pool, off, flen, tcb, np.ones(len(flows), np.uint8))
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all()
    assert (recs["c"]["tcb_idx"] == segs["flow"]).all()
    assert (recs["c"]["datalen"] == lens).all()
    assert (recs["seq"] == segs["seq"]).all() and (recs["ack"] == segs["ack"]).all()


# --------------------------------------------------- the size classes of the test inputs ---
def test_class_lengths_reach_every_class_at_both_ends():
    """From the size-class rule alone (ref.lanes_per_frame, restated from the kernel's header
    comment): CLASS_LENGTHS holds both ends of classes 0-32 and the lower end of class 64, and
    every class whose frames can end inside a round has such a length."""
    ends = {0: (0, 10), 4: (11, 202), 8: (203, 458), 16: (459, 970), 32: (971, 1994), 64: (1995, rxg.TX_MAX_DATA)}
    assert ref.CLASS_RANGE == ends and list(ends) == ref.CLASSES
    for cls, (lo, hi) in ends.items():
        # the ends are ends: one byte less or more is another class
        assert ref.lanes_per_frame(lo) == ref.lanes_per_frame(hi) == cls
        assert lo == 0 or ref.lanes_per_frame(lo - 1) < cls
        assert hi == rxg.TX_MAX_DATA or ref.lanes_per_frame(hi + 1) > cls
        assert lo in ref.CLASS_LENGTHS
        assert hi in ref.CLASS_LENGTHS or cls == 64
    assert all(ref.lanes_per_frame(x) == 64 for x in (2731, 8960, 65481))
    by_class = {c: [x for x in ref.CLASS_LENGTHS if ref.lanes_per_frame(x) == c] for c in ref.CLASSES}
    assert all(by_class.values())
    assert all(ref.chunks_of(x) == 4 * ((54 + x + 63) // 64) for x in ref.CLASS_LENGTHS)
    # a partial last round: NC not a multiple of the lanes per frame.  Class 0 has one round
    # of one line; NC is a multiple of 4 whatever the length, so class 4 has no partial round
    # either: there, a length of several rounds and one of a single round
    for cls in (8, 16, 32, 64):
        assert any(ref.chunks_of(x) % cls for x in by_class[cls]), cls
        assert any(x % 2 and ref.chunks_of(x) % cls for x in by_class[cls]), cls
    assert {ref.chunks_of(x) for x in by_class[4]} >= {8, 16} and any(x % 2 for x in by_class[4])


def test_model_class_lengths_verify_through_the_rx_oracle():
    flows = ref.make_flows()
    r = np.random.default_rng(13)
    lens = np.array(ref.CLASS_LENGTHS)
    payload = r.integers(0, 256, 8192, dtype=np.uint8)
    segs = ref.make_segs(lens, r.integers(0, 8192 - 2731, len(lens)), len(flows), seed=14)
    off, nslots = ref.packed_offsets(lens)
    pool, flen, stats = ref.build(payload, flows, segs, off, nslots)
    assert list(stats) == [len(lens), 0]
    tcb = np.zeros(len(flows), dtype=rxg.TCB_DTYPE)
    tcb["dport"], tcb["sport"] = flows["sport"], flows["dport"]
    tcb["ipv4_dst"] = flows["ipv4_src"].byteswap()
    tcb["ipv4_src"] = flows["ipv4_dst"].byteswap()
    tcb["state"] = rxg.TCP_ESTABLISHED
    recs, _ = oracle.rx_batch(pool, off, flen, tcb, np.ones(len(flows), np.uint8))
    assert (recs["c"]["ip_cksum"] == 0).all() and (recs["c"]["tcp_cksum"] == 0).all()
    assert (recs["c"]["verdict"] == rxg.V_DISPATCH).all()
    assert (recs["c"]["tcb_idx"] == segs["flow"]).all()
    assert (recs["c"]["datalen"] == lens).all()
    assert (recs["seq"] == segs["seq"]).all() and (recs["ack"] == segs["ack"]).all()
    # and the payload bytes are the source's
    for i, L in enumerate(lens):
        a, o = int(off[i]) * 64 + 54, int(segs["src_off"][i])
        assert np.array_equal(pool[a:a + L], payload[o:o + L])
