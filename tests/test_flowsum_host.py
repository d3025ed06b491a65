"""CPU: rxg_flow_sums_host (the per-flow summary of a burst, include/rxg.h) against the numpy
model tests/flowsum_ref.py, and the model against the hand-written vectors of
tests/golden/flowsum_kat.json.  Outputs are pre-filled with 0xA5 and compared whole, eight guard
entries past cap included."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import flowsum_cases as cases
import flowsum_ref as ref
import oracle
import pktgen
import rxg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "flowsum_kat.json")))
# (a vector that names its record kinds or frame lengths is tests/test_flowsum_edge_cases_host.py's)
KATS = [k for k in ALL_KATS if "kinds" not in k]
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
FILL, GUARD, EINVAL = 0xA5, 8, 22


def host_raw(recs, rec_kind, ntcb, frames=None, flags=0, cap=None, n=None):
    """(rc, the whole output buffer of cap + GUARD entries as bytes-filled FLOW_SUM_DTYPE, count)."""
    lib = rxg.load_library()
    recs = np.ascontiguousarray(recs)
    n = recs.nbytes // rec_kind if n is None else n
    cap = n if cap is None else cap
    buf = np.full((cap + GUARD) * 40, FILL, np.uint8)
    count = np.full(3, 0xA5A5A5A5A5A5A5A5, np.uint64)
    keep = [C.create_string_buffer(bytes(f), max(len(f), 1)) for f in frames] if frames is not None else []
    ptrs = (C.c_void_p * max(len(keep), 1))(*[C.addressof(x) for x in keep]) if frames is not None else None
    lens = np.array([len(f) for f in frames], np.uint16) if frames is not None else None
    rc = lib.rxg_flow_sums_host(recs.ctypes.data, rec_kind, ptrs, None if lens is None else lens.ctypes.data, n, ntcb, flags,
                                buf.ctypes.data, cap, count.ctypes.data)
    return rc, buf.view(rxg.FLOW_SUM_DTYPE), count


def check(recs48, rec_kind, ntcb, frames=None, flags=0, cap=None, what=""):
    """The host function on the records in that kind equals the model; returns the model's answer."""
    recs = cases.as_kind(recs48, rec_kind)
    if rec_kind != rxg.REC48 and frames is None:
        frames = cases.frames_for(recs48)
    want, wcount = ref.summaries(recs, rec_kind, ntcb, frames, flags)
    rc, got, count = host_raw(recs, rec_kind, ntcb, frames, flags, cap)
    assert rc == 0, what
    assert count.tolist() == wcount.tolist(), (what, count, wcount)
    cap = len(recs48) if cap is None else cap
    m = min(len(want), cap)
    assert got[:m].tobytes() == want[:m].tobytes(), (what, got[:m], want[:m])
    assert (got[m:].view(np.uint8) == FILL).all(), (what, "entries at or past min(count, cap) were written")
    return want, wcount


def test_struct_layout_matches_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rxg.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u\n", sizeof(rxg_flow_sum),
         offsetof(rxg_flow_sum, tcb_idx), offsetof(rxg_flow_sum, frames), offsetof(rxg_flow_sum, max_seq),
         offsetof(rxg_flow_sum, max_ack), offsetof(rxg_flow_sum, first_idx), offsetof(rxg_flow_sum, last_idx),
         offsetof(rxg_flow_sum, data_frames), offsetof(rxg_flow_sum, tcp_flags_or), offsetof(rxg_flow_sum, state),
         offsetof(rxg_flow_sum, reserved), offsetof(rxg_flow_sum, data_bytes), sizeof(rxg_dev_flow_sums),
         offsetof(rxg_dev_flow_sums, ntcb), offsetof(rxg_dev_flow_sums, count), RXG_FS_TCP_OK_ONLY, RXG_FS_MAX_NTCB);
  return 0;
}'''
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "p.c"), "-o",
                    str(tmp_path / "p")], check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    D, S = rxg.FLOW_SUM_DTYPE, rxg.DevFlowSums
    assert got[0] == 40 == D.itemsize
    assert got[1:12] == [0, 4, 8, 12, 16, 20, 24, 28, 29, 30, 32] == [D.fields[f][1] for f in ref.FIELDS]
    assert got[12:] == [C.sizeof(S), S.ntcb.offset, S.count.offset, rxg.FS_TCP_OK_ONLY, rxg.FS_MAX_NTCB]
    assert C.sizeof(S) == 80


def kat_records(k):
    a = np.array(k["recs"], np.int64)
    return cases.craft(a[:, 0], seq=a[:, 6], ack=a[:, 7], datalen=a[:, 5], tcp_flags=a[:, 3], flags=a[:, 4],
                       verdict=a[:, 1], state=a[:, 2])


@pytest.mark.parametrize("k", KATS, ids=[k["name"] for k in KATS])
@pytest.mark.parametrize("rec_kind", KINDS)
def test_known_answers(k, rec_kind):
    want, count = check(kat_records(k), rec_kind, k["ntcb"], flags=k["flags"], what=k["name"])
    assert [list(ref.as_tuple(w)) for w in want] == k["want"]     # the model gives the hand-written answers
    assert count.tolist() == k["count"]


@pytest.mark.parametrize("rec_kind", KINDS)
def test_maxima_are_unsigned_not_signed_not_serial(rec_kind):
    vals = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
    pairs = [(a, b) for a in vals for b in vals if a != b]
    tcb = np.repeat(np.arange(len(pairs)), 2)
    seq = np.array([v for p in pairs for v in p], np.uint32)
    ack = seq[::-1].copy()
    want, _ = check(cases.craft(tcb, seq=seq, ack=ack), rec_kind, len(pairs))
    assert want["max_seq"].tolist() == [max(p) for p in pairs]
    assert want["max_ack"].tolist() == [max(p) for p in pairs][::-1]


@pytest.mark.parametrize("rec_kind", KINDS)
def test_negative_and_zero_datalen_carry_no_data(rec_kind):
    dl = np.array([-120, -1, 0, 1, 0, 1460, -20], np.int32)
    want, _ = check(cases.craft(np.zeros(len(dl), int), datalen=dl), rec_kind, 4)
    assert (int(want[0]["frames"]), int(want[0]["data_frames"]), int(want[0]["data_bytes"])) == (7, 2, 1461)


def test_data_bytes_pass_2_to_the_32():
    n = 70000
    r = cases.craft(np.full(n, 5), seq=np.arange(n), ack=1, datalen=rxg.TX_MAX_DATA)
    want, _ = check(r, rxg.REC48, 6)
    assert int(want[0]["frames"]) == n and int(want[0]["data_bytes"]) == n * 65481 > 2**32
    assert int(want[0]["last_idx"]) == n - 1 and int(want[0]["max_seq"]) == n - 1


@pytest.mark.parametrize("rec_kind", KINDS)
def test_tcb_idx_edges(rec_kind):
    for ntcb in (100, cases.REC8_MAX_TCB, cases.REC8_MAX_TCB + 1, rxg.FS_MAX_NTCB):
        tcb = np.array([-1, ntcb - 1, ntcb, cases.REC8_MAX_TCB, 0, ntcb - 1])
        tcb = tcb[tcb <= cases.REC8_MAX_TCB]
        want, count = check(cases.craft(tcb, seq=np.arange(len(tcb))), rec_kind, ntcb, what=f"ntcb {ntcb}")
        inr = (tcb >= 0) & (tcb < ntcb)
        assert int(count[1]) == int((~inr).sum()) >= 1 and int(count[2]) == 0
        assert want["tcb_idx"].tolist() == sorted(set(tcb[inr].tolist()))


@pytest.mark.parametrize("rec_kind", KINDS)
def test_tcp_ok_only_on_and_off(rec_kind):
    fl = np.array([cases.OK, rxg.F_IP_OK, cases.OK, rxg.F_IP_OK, 0, cases.OK], np.uint8)
    r = cases.craft([2, 2, 7, 9, 9, 50], seq=[1, 99, 3, 4, 5, 6], flags=fl)
    off, c0 = check(r, rec_kind, 40, flags=0)
    on, c1 = check(r, rec_kind, 40, flags=rxg.FS_TCP_OK_ONLY)
    # tcb 50 is out of range either way; frames 1, 3 and 4 lack RXG_F_TCP_OK (flow 9 loses both of its)
    assert c0.tolist() == [3, 1, 0] and c1.tolist() == [2, 1, 3]
    assert off["tcb_idx"].tolist() == [2, 7, 9] and on["tcb_idx"].tolist() == [2, 7]
    assert int(off[0]["max_seq"]) == 99 and int(on[0]["max_seq"]) == 1


@pytest.mark.parametrize("rec_kind", [rxg.REC8, rxg.REC16])
def test_frames_cut_inside_seq_and_ack_read_zero_past_len(rec_kind):
    lens = [0] + list(range(38, 47)) + [54]
    r = cases.craft(np.arange(len(lens)), seq=0xA1B2C3D4, ack=0xE5F60718)
    frames = cases.frames_for(r, lens)
    assert [len(f) for f in frames] == lens
    want, _ = check(r, rec_kind, len(lens), frames)
    assert want["max_seq"].tolist() == [0, 0, 0xA1000000, 0xA1B20000, 0xA1B2C300] + [0xA1B2C3D4] * 6
    assert want["max_ack"].tolist() == [0] * 6 + [0xE5000000, 0xE5F60000, 0xE5F60700, 0xE5F60718, 0xE5F60718]


@pytest.mark.parametrize("rec_kind", KINDS)
def test_cap_cuts_the_output_not_the_count(rec_kind):
    rng = np.random.default_rng(5)
    r = cases.craft(rng.integers(0, 23, 300), seq=rng.integers(0, 2**32, 300), ack=rng.integers(0, 2**32, 300),
                    datalen=rng.integers(-5, 50, 300))
    m = len(np.unique(r["c"]["tcb_idx"]))
    for cap in (0, m - 1, m, m + 1):
        _, count = check(r, rec_kind, 23, cap=cap, what=f"cap {cap}")
        assert int(count[0]) == m


def test_argument_errors():
    lib = rxg.load_library()
    r = cases.as_kind(cases.craft([1, 2]), rxg.REC16)
    frames = cases.frames_for(cases.craft([1, 2]))
    assert host_raw(r, rxg.REC16, 8, frames)[0] == 0
    for kw in (dict(rec_kind=0), dict(rec_kind=32), dict(ntcb=0), dict(ntcb=rxg.FS_MAX_NTCB + 1), dict(flags=2),
               dict(flags=0x80000001), dict(frames=None)):
        a = dict(recs=r, rec_kind=rxg.REC16, ntcb=8, frames=frames, flags=0, n=2)
        a.update(kw)
        rc, got, count = host_raw(**a)
        assert rc == -EINVAL, kw
        assert (got.view(np.uint8) == FILL).all() and (count == 0xA5A5A5A5A5A5A5A5).all(), kw
    out, count = np.zeros(4, rxg.FLOW_SUM_DTYPE), np.zeros(3, np.uint64)
    ptrs = (C.c_void_p * 2)()
    lens = np.zeros(2, np.uint16)
    args = lambda **kw: [kw.get("recs", r.ctypes.data), 16, kw.get("frames", ptrs), kw.get("lens", lens.ctypes.data), 2, 8, 0,
                         kw.get("out", out.ctypes.data), kw.get("cap", 4), kw.get("count", count.ctypes.data)]
    assert lib.rxg_flow_sums_host(*args(recs=None)) == -EINVAL
    assert lib.rxg_flow_sums_host(*args(count=None)) == -EINVAL
    assert lib.rxg_flow_sums_host(*args(out=None)) == -EINVAL
    assert lib.rxg_flow_sums_host(*args(lens=None)) == -EINVAL
    assert lib.rxg_flow_sums_host(*args(out=None, cap=0)) == 0 and int(count[0]) == 2
    # REC48 needs no frames; n == 0 writes the three zeroes and nothing else
    r48 = cases.craft([1, 2])
    assert host_raw(r48, rxg.REC48, 8)[0] == 0
    rc, got, count = host_raw(r48, rxg.REC48, 8, n=0, cap=4)
    assert rc == 0 and count.tolist() == [0, 0, 0] and (got.view(np.uint8) == FILL).all()


def test_binding_wrapper_matches_the_raw_call():
    r = cases.craft([4, 4, 1], seq=[5, 9, 2], datalen=[0, 10, 0])
    sums, count = rxg.flow_sums_host(cases.as_kind(r, rxg.REC8), rxg.REC8, 8, cases.frames_for(r))
    want, wcount = ref.summaries(r, rxg.REC48, 8)
    assert sums.tobytes() == want.tobytes() and count.tolist() == wcount.tolist()


def test_parity_set_in_all_three_kinds():
    rows, frames = pktgen.parity_set(seed=31, n=3000)
    tcb, live = pktgen.table_arrays(rows)
    exp, _ = oracle.rx_batch(*pktgen.pack_arena(frames), tcb, live)
    c = exp["c"]
    assert (c["verdict"] == rxg.V_DISPATCH).sum() > 300 and ((c["flags"] & rxg.F_TCP_OK) == 0).any()
    for flags in (0, rxg.FS_TCP_OK_ONLY):
        got = [check(exp, k, len(rows), frames, flags, what=f"records of {k}") for k in KINDS]
        assert got[0][0].tobytes() == got[1][0].tobytes() == got[2][0].tobytes()
        assert got[0][1].tolist() == got[1][1].tolist() == got[2][1].tolist()
        assert len(got[0][0]) > 20 and (got[0][0]["data_frames"] > 0).any()
    assert int(got[0][1][2]) > 0     # the checksum flag left frames out
