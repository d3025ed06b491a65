"""The flow-train rule of include/rxg.h (rxg_flow_trains_dev / rxg_flow_trains_host) restated in
numpy: a lexsort, then "continues its predecessor" per sorted segment and a reduction per run.
What the tests expect, never taken from the code under test; the rule's claims about the
reference are checked against oracle/window.py in tests/test_flowtrain_host.py."""
import numpy as np

import rxg
from flowsum_ref import decode, seq_ack

FIN = 0x01
M32 = 0xFFFFFFFF


def segments(recs, rec_kind, ntcb, frames=None, flags=0):
    """(idx, tcb, seq, datalen, fin) of the burst's segments in packet order, and count[2], count[3]."""
    c = decode(recs, rec_kind)
    n = len(c)
    seq = seq_ack(recs, rec_kind, frames)[0] if n else np.zeros(0, np.uint32)
    tcb = c["tcb_idx"].astype(np.int64)
    dl = c["datalen"].astype(np.int64)
    disp = c["verdict"] == rxg.V_DISPATCH
    inr = disp & (tcb >= 0) & (tcb < ntcb)
    ok = np.ones(n, bool) if not (flags & rxg.FT_TCP_OK_ONLY) else (c["flags"] & rxg.F_TCP_OK) != 0
    seg = inr & ok & (dl > 0) & (dl <= 65535)
    idx = np.nonzero(seg)[0]
    return (idx, tcb[idx], seq[idx].astype(np.int64), dl[idx], (c["tcp_flags"][idx] & FIN) != 0,
            int((disp & ~inr).sum()), int((inr & ~ok).sum()))


def trains(recs, rec_kind, ntcb, frames=None, flags=0, cur_seq=None):
    """(order u32[S], FLOW_TRAIN_DTYPE[T], count u64[4]): everything, whatever a cap would be."""
    idx, tcb, seq, dl, fin, nout, nleft = segments(recs, rec_kind, ntcb, frames, flags)
    o = np.lexsort((idx, tcb))                 # tcb_idx ascending, packet index ascending
    idx, tcb, seq, dl, fin = idx[o], tcb[o], seq[o], dl[o], fin[o]
    S = len(idx)
    t = np.zeros(0, rxg.FLOW_TRAIN_DTYPE)
    if S:
        wraps = seq + dl >= 1 << 32
        cont = np.zeros(S, bool)               # segment k continues segment k - 1
        cont[1:] = ((tcb[1:] == tcb[:-1]) & (seq[1:] == ((seq[:-1] + dl[:-1]) & M32)) & ~fin[:-1] & ~wraps[:-1]
                    & ~wraps[1:])
        first = np.nonzero(~cont)[0]
        end = np.append(first[1:], S)          # one past each train's last segment
        nbytes = np.add.reduceat(dl, first)
        new_flow = np.ones(S + 1, bool)        # segment k is its flow's first (k == S: past the list)
        new_flow[1:S] = tcb[1:] != tcb[:-1]
        t = np.zeros(len(first), rxg.FLOW_TRAIN_DTYPE)
        t["tcb_idx"], t["first"], t["nseg"], t["seq"], t["bytes"] = tcb[first], first, end - first, seq[first], nbytes
        t["next_ack"] = (((seq[first] + nbytes) & M32) + fin[end - 1]) & M32
        fl = (np.where(fin[end - 1], rxg.FTR_FIN, 0) | np.where(wraps[first], rxg.FTR_WRAP, 0) |
              np.where(new_flow[first], rxg.FTR_FLOW_FIRST, 0) | np.where(new_flow[end], rxg.FTR_FLOW_LAST, 0))
        if cur_seq is not None:
            cur = np.asarray(cur_seq, np.int64)[tcb[first]]
            fl |= np.where(new_flow[first] & ~wraps[first] & (cur != 0) & (cur == seq[first]), rxg.FTR_HEAD, 0)
        t["flags"] = fl
    return idx.astype(np.uint32), t, np.array([S, len(t), nout, nleft], np.uint64)
