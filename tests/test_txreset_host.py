"""CPU: the device reset build's host side -- the reference model the GPU tests compare with
(tests/txreset_ref.py) pinned against one reset written out byte by byte and against the
receive oracle, rxg_reset_set_id against rebuilding with the new id (in Python and stand-alone
under ASan/UBSan), and rxg_dev_tx_reset / the new entry points at the C boundary."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import oracle
import pktgen
import rxg
import txreset_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
EINVAL = 22
NEW = ("rxg_tx_reset_dev", "rxg_reset_set_id", "rxg_reset_attach", "rxg_reset_take")


@pytest.fixture(scope="module", autouse=True)
def library_has_the_reset_entry_points():
    """The model pinned here describes a call of the library under test: without that call
    nothing in this file says anything about it."""
    lib = rxg.load_library()
    missing = [name for name in NEW if not hasattr(lib, name)]
    assert not missing, missing


# ------------------------------------------------------------------- 1. the model pin ---
def hand_offender() -> bytes:
    """54 bytes put together field by field: 172.16.5.9:40001 -> 192.168.78.2:9999, ACK."""
    eth = bytes([0x02, 0, 0xC0, 0xA8, 0x4E, 0x02]) + bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55]) + b"\x08\x00"
    ip = struct.pack("!BBHHHBBH", 0x45, 0, 40, 0x1234, 0x4000, 64, 6, 0) + bytes([172, 16, 5, 9]) + bytes([192, 168, 78, 2])
    tcp = struct.pack("!HHIIBBHHH", 40001, 9999, 0x01020304, 0xA1B2C3D4, 0x50, 0x10, 0xFFFF, 0, 0)
    f = eth + ip + tcp
    assert len(f) == 54
    return f


def test_model_equals_a_reset_written_out_by_hand():
    ip_id = 0x0102
    want = bytearray(64)
    want[0:6] = bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55])   # the offender's source MAC
    want[6:12] = bytes([0x6A, 0x9C, 0xBA, 0xA0, 0x96, 0x24])  # etherout.c:94-99
    want[12:14] = b"\x08\x00"
    want[14:16] = b"\x45\x00"
    want[16:18] = b"\x00\x28"                                 # htons(40)
    want[18:20] = b"\x02\x01"                                 # 0x0102 stored by an x86 (ip.c:106)
    want[20:22] = b"\x00\x00"
    want[22:24] = b"\x7f\x06"
    want[26:30] = bytes([192, 168, 78, 2])
    want[30:34] = bytes([172, 16, 5, 9])
    want[34:36] = (9999).to_bytes(2, "big")
    want[36:38] = (40001).to_bytes(2, "big")
    want[38:42] = bytes([0xA1, 0xB2, 0xC3, 0xD4])             # the offender's recv_ack
    want[42:46] = bytes(4)
    want[46:48] = b"\x50\x04"
    want[48:50] = b"\xe0\x2e"                                 # 12000 = 0x2EE0 stored by an x86
    want[52:54] = b"\x00\x00"
    ipck = oracle.calculate_checksum(bytes(want[14:34]))
    want[24:26] = ipck.to_bytes(2, "big")
    pseudo = bytes(want[26:34]) + b"\x00\x06" + (20).to_bytes(2, "big")
    tck = oracle.calculate_checksum(pseudo + bytes(want[34:54]))
    want[50:52] = tck.to_bytes(2, "big")
    got = ref.one(hand_offender(), ip_id)
    assert got == bytes(want), [(i, got[i], want[i]) for i in range(64) if got[i] != want[i]]
    # the pure-Python RFC 1071 sum agrees with the oracle's on this header
    assert pktgen.py_checksum(bytes(want[14:24]) + b"\0\0" + bytes(want[26:34])) == ipck
    # through build(): the same line, index and count
    arena, off, lens = pktgen.pack_arena([b"\xff" * 60, hand_offender()])
    out, idx, count = ref.build(arena, off, lens, [rxg.V_DROP_L2, rxg.V_RST_NOPCB], ip_id, rxg.REF_SRC_MAC, 8)
    assert count == 1 and idx.tolist() == [1] and out.tobytes() == bytes(want)


def test_model_resets_verify_through_the_rx_oracle():
    rows, frames = pktgen.parity_set(seed=77, n=3000)
    tcb, live = pktgen.table_arrays(rows)
    arena, off, lens = pktgen.pack_arena(frames)
    recs, _ = oracle.rx_batch(arena, off, lens, tcb, live)
    v = recs["c"]["verdict"]
    out, idx, count = ref.build(arena, off, lens, v, 0xFFF0, rxg.REF_SRC_MAC, 1 << 20)
    assert count == len(idx) == int(np.isin(v, ref.RST_VERDICTS).sum()) and count > 200
    assert (v[idx] == rxg.V_RST_NOPCB).any() and (v[idx] == rxg.V_RST_LISTEN_NONSYN).any()
    assert (recs["c"]["flags"][idx] & rxg.F_TRUNC).any()  # truncated offenders are in the set
    back, _ = oracle.rx_batch(out, np.arange(count, dtype=np.uint32), np.full(count, 54, np.uint16), tcb[:0])
    assert (back["c"]["ip_cksum"] == 0).all() and (back["c"]["tcp_cksum"] == 0).all()
    assert (back["c"]["verdict"] == rxg.V_RST_NOPCB).all() and (back["c"]["tcp_flags"] == rxg.TCP_FLAG_RST).all()
    o = recs[idx]  # the offenders: the reset's 4-tuple is theirs mirrored
    assert np.array_equal(back["sport"], o["dport"]) and np.array_equal(back["dport"], o["sport"])
    assert np.array_equal(back["src_ip"], o["dst_ip_raw"].byteswap())
    assert np.array_equal(back["dst_ip_raw"], o["src_ip"].byteswap())
    assert np.array_equal(back["seq"], o["ack"]) and (back["ack"] == 0).all()
    assert np.array_equal(back["src_mac"], np.tile(np.frombuffer(rxg.REF_SRC_MAC, np.uint8), (count, 1)))
    lines = out.reshape(count, 64)
    assert np.array_equal(lines[:, 0:6], o["src_mac"])
    ids = lines[:, 18].astype(np.uint32) | (lines[:, 19].astype(np.uint32) << 8)
    assert np.array_equal(ids, (0xFFF0 + np.arange(count)) & 0xFFFF)  # wraps at 16 bits
    assert not lines[:, 54:].any()


# --------------------------------------------------------------- 2. rxg.reset_set_id ---
IDS = [0, 1, 0x00FF, 0xFF00, 0xFFFF]


def corner_offender(ip_id: int) -> bytes:
    """An offender whose reset with packet_id ip_id has a header sum that folds to 0xFFFF: the
    low half of its source address (the reset's dst_addr, the header's last word) is chosen so
    that the big-endian words add up to a multiple of 0xFFFF; the checksum is then 0x0000."""
    f = bytearray(hand_offender())
    f[28:30] = b"\0\0"
    line = ref.reset_unsummed(bytes(f) + bytes(10), ip_id, rxg.REF_SRC_MAC)
    s = sum(struct.unpack("!10H", bytes(line[14:34])))
    f[28:30] = ((0xFFFF - s % 0xFFFF) % 0xFFFF).to_bytes(2, "big")
    return bytes(f)


@pytest.mark.parametrize("ip_id", IDS)
def test_reset_set_id_equals_rebuilding(ip_id):
    for inb in (hand_offender(), corner_offender(ip_id)):
        for old in (0x0102, ip_id, (ip_id + 1) & 0xFFFF):
            built = ref.one(inb, old)
            want = ref.one(inb, ip_id)
            assert rxg.reset_set_id(built, ip_id) == want
            a = np.frombuffer(built, np.uint8).copy()
            assert rxg.reset_set_id(a, ip_id) == want and a.tobytes() == want  # in place
    corner = ref.one(corner_offender(ip_id), ip_id)
    assert corner[24:26] == b"\0\0"  # the 0x0000 / 0xFFFF corner is reached
    assert oracle.calculate_checksum(corner[14:24] + b"\0\0" + corner[26:34]) == 0


# --------------------------------------- 3. rxg_reset_set_id stand-alone, sanitized too ---
@pytest.mark.parametrize("san", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_reset_set_id_standalone(tmp_path, san):
    exe = tmp_path / "txreset_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *san, "-I", INC,
                    os.path.join(ROOT, "tests", "txreset_check.cpp"),
                    os.path.join(ROOT, "dpdk-tcpipstack_amd", "csrc", "rxg_txresetid.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "txreset ok" in r.stdout and not r.stderr.strip(), r.stdout + r.stderr


# ------------------------------------------------- 4. layouts, exports, NULL arguments ---
PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "rxg.h"
#define O(f) printf(#f " %zu\n", offsetof(rxg_dev_tx_reset, f))
int main(void)
{
    printf("sizeof %zu\n", sizeof(rxg_dev_tx_reset));
    O(frames); O(off64); O(len); O(slot0); O(stride64); O(n); O(rec_kind); O(recs); O(out); O(idx); O(cap);
    O(count); O(ip_id0); O(src_mac);
    printf("abi %d\n", RXG_ABI_VERSION);
    return 0;
}
"""


def test_struct_layout_by_c_probe(tmp_path):
    (tmp_path / "probe.c").write_text(PROBE)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", INC, str(tmp_path / "probe.c"), "-o",
                    str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.strip().splitlines())
    assert int(got.pop("sizeof")) == C.sizeof(rxg.DevTxReset) == 88
    assert int(got.pop("abi")) == rxg.ABI_VERSION == 2
    assert sorted(got) == sorted(f for f, *_ in rxg.DevTxReset._fields_)
    for f, off in got.items():
        assert int(off) == getattr(rxg.DevTxReset, f).offset, f
    assert rxg.TX_RESET is rxg.DevTxReset


def test_declared_exported_and_null_arguments():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INC, "rxg.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
    out = subprocess.run(["nm", "-D", "--defined-only", rxg.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert set(NEW) <= set(re.findall(r"\bT (\w+)", out))
    lib = rxg.load_library()
    b = rxg.DevTxReset()
    assert lib.rxg_tx_reset_dev(None, C.byref(b), None) == -EINVAL and b"NULL" in lib.rxg_last_error()
    p = C.c_void_p()
    assert lib.rxg_reset_take(None, 0, C.byref(p)) == -EINVAL
    assert lib.rxg_reset_attach(None, None, None, 0) == -EINVAL
    lib.rxg_reset_set_id(None, 5)  # a NULL line is left alone
