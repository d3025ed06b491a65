"""The per-flow summary rule of include/rxg.h (rxg_flow_sums_dev / rxg_flow_sums_host) restated in
numpy: what the tests expect, never taken from the code under test.  Pinned by the hand-written
vectors of tests/golden/flowsum_kat.json (tests/test_flowsum_host.py)."""
import numpy as np

import rxg

FIELDS = ["tcb_idx", "frames", "max_seq", "max_ack", "first_idx", "last_idx", "data_frames", "tcp_flags_or", "state",
          "reserved", "data_bytes"]


def decode(recs, rec_kind):
    """The burst's records as REC16_DTYPE (rxg_rec8 as rxg_rec8_expand gives them)."""
    recs = np.ascontiguousarray(recs)
    if rec_kind == rxg.REC8:
        return rxg.rec8_expand(recs.view(rxg.REC8_DTYPE))
    if rec_kind == rxg.REC16:
        return recs.view(rxg.REC16_DTYPE).copy()
    return recs.view(rxg.REC48_DTYPE)["c"].copy()


def be32_cut(frame: bytes, at: int) -> int:
    """Big-endian frame[at .. at + 4), bytes at or beyond the frame's end read as zero."""
    return int.from_bytes((bytes(frame[at:at + 4]) + b"\0\0\0\0")[:4], "big")


def seq_ack(recs, rec_kind, frames=None):
    """(seq, ack) per frame: the record's for REC48, frame[38..42) / frame[42..46) otherwise."""
    if rec_kind == rxg.REC48:
        r = np.ascontiguousarray(recs).view(rxg.REC48_DTYPE)
        return r["seq"].astype(np.uint32), r["ack"].astype(np.uint32)
    return (np.array([be32_cut(f, 38) for f in frames], np.uint32),
            np.array([be32_cut(f, 42) for f in frames], np.uint32))


def summaries(recs, rec_kind, ntcb, frames=None, flags=0):
    """(FLOW_SUM_DTYPE array of every touched flow in ascending tcb_idx, count u64[3])."""
    c = decode(recs, rec_kind)
    n = len(c)
    seq, ack = seq_ack(recs, rec_kind, frames) if n else (np.zeros(0, np.uint32),) * 2
    tcb = c["tcb_idx"].astype(np.int64)
    disp = c["verdict"] == rxg.V_DISPATCH
    inr = disp & (tcb >= 0) & (tcb < ntcb)
    ok = np.ones(n, bool) if not (flags & rxg.FS_TCP_OK_ONLY) else (c["flags"] & rxg.F_TCP_OK) != 0
    counted = inr & ok
    idx = np.nonzero(counted)[0]
    flows = np.unique(tcb[idx])
    k = np.searchsorted(flows, tcb[idx])
    m = len(flows)
    frames_n, dfr = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    mseq, mack = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    first, last = np.full(m, 0xFFFFFFFF, np.uint32), np.zeros(m, np.uint32)
    orf, nbytes = np.zeros(m, np.uint8), np.zeros(m, np.uint64)
    np.add.at(frames_n, k, 1)
    np.maximum.at(mseq, k, seq[idx])
    np.maximum.at(mack, k, ack[idx])
    np.minimum.at(first, k, idx.astype(np.uint32))
    np.maximum.at(last, k, idx.astype(np.uint32))
    np.bitwise_or.at(orf, k, c["tcp_flags"][idx])
    dl = c["datalen"][idx].astype(np.int64)
    pos = dl > 0
    np.add.at(dfr, k[pos], 1)
    np.add.at(nbytes, k[pos], dl[pos].astype(np.uint64))
    out = np.zeros(m, rxg.FLOW_SUM_DTYPE)
    out["tcb_idx"], out["frames"], out["max_seq"], out["max_ack"] = flows, frames_n, mseq, mack
    out["first_idx"], out["last_idx"], out["data_frames"], out["tcp_flags_or"] = first, last, dfr, orf
    out["state"] = c["state"][first.astype(np.int64)] if m else 0
    out["data_bytes"] = nbytes
    count = np.array([m, int((disp & ~inr).sum()), int((inr & ~ok).sum())], np.uint64)
    return out, count


def as_tuple(s):
    return tuple(int(s[f]) for f in FIELDS)
