"""The train-payload rule of include/rxg.h (rxg_train_payload_dev / rxg_train_payload_host)
restated in numpy on top of flowtrain_ref.trains.  What the tests expect, never taken from the
code under test; what the rule promises about the reference's receive window is checked against
oracle/window.py in tests/test_trainpay_host.py.

The burst's frames are a pool: frame i is pool[64 * off64[i] .. + lens[i])."""
import numpy as np

import rxg
from flowsum_ref import decode

M32 = 0xFFFFFFFF
MAXCAND = 2  # the highest verdict whose payload is gathered: RST_LISTEN_NONSYN


def pad16(b):
    return (b + 15) // 16 * 16


def frame_seq(pool, off64, lens, recs, rec_kind):
    """seq per frame as rxg_flow_trains_dev reads it: REC48's own, else big-endian frame[38..42)
    with bytes at or beyond the frame's length read as zero."""
    if rec_kind == rxg.REC48:
        return np.ascontiguousarray(recs).view(rxg.REC48_DTYPE)["seq"].astype(np.int64)
    base = off64.astype(np.int64) * 64
    seq = np.zeros(len(off64), np.int64)
    for k in range(4):
        b = np.where(lens > 38 + k, pool[np.minimum(base + 38 + k, len(pool) - 1)], 0).astype(np.int64)
        seq = (seq << 8) | b
    return seq


def gather(pool, off64, lens, recs, rec_kind, order, trains, count, cap_seg, cap_trains, flags, arena, arena_cap,
           want_msgs=True, want_tmsgs=True):
    """(arena after the call, msgs[n] or None, tmsgs[cap_trains] after the call or None, arena_used).
    arena: what the buffer held before (a copy is written); order and trains are the whole lists
    (the caps cut them here, as the buffers would)."""
    c = decode(recs, rec_kind)
    n = len(c)
    arena = arena.copy()
    msgs = np.zeros(n, rxg.PAYLOAD_MSG_DTYPE) if want_msgs else None
    S = min(int(count[0]), cap_seg, n)
    T = 0 if S == 0 else min(int(count[1]), cap_trains, n)
    tm = np.zeros(T, rxg.PAYLOAD_MSG_DTYPE)
    if n == 0:
        return arena, None if msgs is None else msgs, tm if want_tmsgs else None, 0
    off64, lens = off64.astype(np.int64), lens.astype(np.int64)
    seq = frame_seq(pool, off64, lens, recs, rec_kind)
    t = trains[:T]
    first, nseg, nbytes = t["first"].astype(np.int64), t["nseg"].astype(np.int64), t["bytes"].astype(np.int64)
    takes = (first + nseg <= S) & (nbytes <= M32)
    if flags & rxg.TP_HEAD_ONLY:
        takes &= (t["flags"] & rxg.FTR_HEAD) != 0
    size = np.where(takes, pad16(nbytes), 0)
    toff = np.cumsum(size) - size
    used = int(size.sum())
    placed = takes & (toff + size <= arena_cap)
    tm["arena_off"] = np.where(placed, toff, 0)
    tm["len"] = np.where(placed, nbytes, 0)
    tm["flags"] = np.where(placed, rxg.PM_GATHERED, 0)
    # one row per segment of a placed train
    k = np.repeat(np.nonzero(placed)[0], nseg[placed])
    j = np.concatenate([np.arange(a, a + b) for a, b in zip(first[placed], nseg[placed])]) if len(k) else np.zeros(0, np.int64)
    i = order[j].astype(np.int64) if len(j) else np.zeros(0, np.int64)
    ok = i < n
    ic = np.where(ok, i, 0)
    dl = c["datalen"][ic].astype(np.int64)
    flen = lens[ic]
    doff = pool[np.minimum(off64[ic] * 64 + 46, len(pool) - 1)].astype(np.int64) >> 4
    start = 34 + doff * 4
    rel = (seq[ic] - t["seq"][k].astype(np.int64)) & M32
    cand = (ok & (c["verdict"][ic] <= MAXCAND) & (dl > 0) & ((c["flags"][ic] & rxg.F_TRUNC) == 0) & (flen > 46)
            & (start + dl <= flen) & (rel + dl <= nbytes[k]))
    hole = np.zeros(T, bool)
    hole[k[~cand]] = True
    tm["flags"] |= np.where(hole, rxg.PM_HOLE, 0).astype(np.uint32)
    ci = ic[cand]
    cdl, cdst, csrc = dl[cand], (toff[k] + rel)[cand], (off64[ic] * 64 + start)[cand]
    if len(ci):
        tot = int(cdl.sum())
        within = np.arange(tot) - np.repeat(np.cumsum(cdl) - cdl, cdl)
        arena[np.repeat(cdst, cdl) + within] = pool[np.repeat(csrc, cdl) + within]
        if msgs is not None:
            msgs["arena_off"][ci] = cdst
            msgs["len"][ci] = cdl
            msgs["flags"][ci] = rxg.PM_GATHERED | np.where(cdl >= 1000, rxg.PM_REF_OVERSIZE, 0)
    for a, b in zip((toff + nbytes)[placed].tolist(), (toff + size)[placed].tolist()):
        arena[a:b] = 0
    return arena, msgs, tm if want_tmsgs else None, used
