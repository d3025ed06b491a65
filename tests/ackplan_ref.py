"""Reference model of the ACK plan (rxg_ack_plan_dev / rxg_ack_plan_host), written from the rule's
text in include/rxg.h, not from the C++: plain Python over numpy arrays, one flow at a time."""
import numpy as np

import rxg

M32 = 0xFFFFFFFF


def bounds(train_count, cap_seg, cap_trains, n):
    """S' and T' (rxg.h): min(count, cap, n), T' = 0 when S' == 0."""
    S = min(int(train_count[0]), cap_seg, n)
    T = min(int(train_count[1]), cap_trains, n) if S else 0
    return S, T


def ts_block(tsval, tsecr):
    """The 48 bytes rxg_tx_opt_timestamp defines: len 12, 01 01 08 0A TSval TSecr, the rest zero."""
    o = np.zeros(1, dtype=rxg.TX_OPT_DTYPE)
    o["len"] = 12
    o["bytes"][0, :12] = np.frombuffer(bytes([1, 1, 8, 10]) + (tsval & M32).to_bytes(4, "big") +
                                       (tsecr & M32).to_bytes(4, "big"), np.uint8)
    return o[0]


def plan(order, trains, train_count, n, ntcb, state, rxopts=None, tsval_now=0, ip_id0=0, opt_plain=0, opt_base=0,
         opt_cap=0, opts=None, cap=None, cap_seg=None, cap_trains=None):
    """(segs, acks, count u64[4], blocks) with segs / acks the min(count[0], cap) entries written
    and blocks {index into opts: the block written there}.  state is indexed only inside
    [0, ntcb), order only below S', rxopts only below n."""
    cap_seg = len(order) if cap_seg is None else cap_seg
    cap_trains = len(trains) if cap_trains is None else cap_trains
    cap = len(trains) if cap is None else cap
    S, T = bounds(train_count, cap_seg, cap_trains, n)
    segs, acks, blocks = [], [], {}
    count = [0, 0, 0, 0]
    tcb = trains["tcb_idx"].tolist()
    a = 0
    for k in range(T):
        if k and tcb[k - 1] == tcb[k]:
            continue                                    # a later train of the same flow
        idx = tcb[k]
        if not 0 <= idx < ntcb:
            count[2] += 1
            continue
        st = state[idx]
        if not int(st["flags"]) & rxg.AS_LIVE:
            count[1] += 1
            continue
        h = trains[k]
        adv = bool(int(h["flags"]) & rxg.FTR_HEAD)
        if adv:
            ack, fl = int(h["next_ack"]), rxg.ACK_ADVANCES | (rxg.ACK_FIN if int(h["flags"]) & rxg.FTR_FIN else 0)
        else:
            ack, fl = int(st["rcv_ack"]), rxg.ACK_DUP
        reserved = opt_plain
        if int(st["flags"]) & rxg.AS_TS and opts is not None:
            if opt_base + a < opt_cap:
                tsecr = int(st["ts_recent"])
                first = int(h["first"])
                if adv and rxopts is not None and first < S:
                    pkt = int(order[first])
                    if pkt < n and int(rxopts[pkt]["flags"]) & rxg.O_TS:
                        tsecr = int(rxopts[pkt]["tsval"])
                reserved = opt_base + a + 1
                if a < cap:
                    blocks[opt_base + a] = ts_block(tsval_now, tsecr)
            else:
                fl |= rxg.ACK_NO_OPT
                count[3] += 1
        if a < cap:
            segs.append((0, idx, int(st["snd_nxt"]), ack, 0, int(st["win_raw"]), (ip_id0 + a) & 0xFFFF, 0x10, 0, reserved))
            acks.append((idx, ack, int(st["snd_nxt"]), fl | ((k & 0xFFFFFF) << 8)))
        a += 1
    count[0] = a
    return (np.array(segs, dtype=rxg.TX_SEG_DTYPE), np.array(acks, dtype=rxg.ACK_DTYPE),
            np.array(count, dtype=np.uint64), blocks)
