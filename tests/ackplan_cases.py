"""Deterministic inputs for the ACK plan (rxg_ack_plan_dev / rxg_ack_plan_host).  The call is a pure
function of its arguments, so trains, counts, state and rxopts are written here directly.  Every set
is small; the largest is 65 537 trains (2 MB).  expect(s) gives the whole output buffers -- segs,
acks, opts, count, each pre-filled with 0xA5 and with guard entries past the last written one -- as
tests/ackplan_ref.py's model says they must stand after the call."""
import numpy as np

import ackplan_ref as ref
import rxg

FILL, GUARD = 0xA5, 4
TILE, SCAN = rxg.ACK_PLAN_TILE, rxg.ACK_PLAN_SCAN_TILES
ROUND = TILE * SCAN                       # trains one round of the scan covers
POISON = 4                                # state entries past ntcb, LIVE | TS: an ACK if ever read
HEAD, FIN, FIRST, LAST = rxg.FTR_HEAD, rxg.FTR_FIN, rxg.FTR_FLOW_FIRST, rxg.FTR_FLOW_LAST
LIVE, TS = rxg.AS_LIVE, rxg.AS_TS


class Set:
    def __init__(self, name, tcb, flags, next_ack, state, ntcb, order=None, n=None, rxopts=None, use_opts=True,
                 first=None, nseg=1, **args):
        T = len(tcb)
        self.name = name
        self.trains = np.zeros(T, dtype=rxg.FLOW_TRAIN_DTYPE)
        self.trains["tcb_idx"] = tcb
        self.trains["first"] = np.arange(T) if first is None else first
        self.trains["nseg"] = nseg
        self.trains["seq"] = 1000
        self.trains["bytes"] = 100
        self.trains["next_ack"] = next_ack
        self.trains["flags"] = flags
        self.order = np.arange(T, dtype=np.uint32) if order is None else np.asarray(order, dtype=np.uint32)
        self.n = T if n is None else n
        self.train_count = np.array([len(self.order), T, 0, 0], dtype=np.uint64)
        self.ntcb = ntcb
        self.state = np.zeros(ntcb + POISON, dtype=rxg.ACK_STATE_DTYPE)
        self.state[:ntcb] = state
        self.state[ntcb:] = (0xDEAD0001, 0xDEAD0002, 0xDEAD0003, 0xDEAD, LIVE | TS)
        self.rxopts = rxopts
        self.use_opts = use_opts
        self.args = dict(tsval_now=0x01020304, ip_id0=7, opt_plain=0, opt_base=0, opt_cap=None, cap=None,
                         cap_seg=len(self.order), cap_trains=T)
        self.args.update(args)
        if self.args["cap"] is None:
            self.args["cap"] = T
        if self.args["opt_cap"] is None:
            self.args["opt_cap"] = self.args["opt_base"] + T
        # the caller's constant blocks: never touched
        self.const = np.zeros(self.args["opt_base"], dtype=rxg.TX_OPT_DTYPE)
        for k in range(len(self.const)):
            self.const[k] = rxg.tx_opt_ref_ack()[0] if k == 0 else ref.ts_block(k, k)

    def variant(self, suffix, **over):
        s = Set.__new__(Set)
        s.__dict__.update(self.__dict__)
        s.name = f"{self.name} {suffix}"
        s.args = dict(self.args)
        for k in ("train_count", "rxopts", "use_opts", "n"):
            if k in over:
                setattr(s, k, over.pop(k))
        s.args.update(over)
        return s

    def model(self):
        a = self.args
        return ref.plan(self.order, self.trains, self.train_count, self.n, self.ntcb, self.state, self.rxopts,
                        a["tsval_now"], a["ip_id0"], a["opt_plain"], a["opt_base"], a["opt_cap"],
                        self.opts_in() if self.use_opts else None, a["cap"], a["cap_seg"], a["cap_trains"])

    def opts_in(self):
        """The option table as the caller hands it over: its constants, then 0xA5."""
        o = np.full((self.args["opt_cap"] + GUARD) * 48, FILL, np.uint8).view(rxg.TX_OPT_DTYPE)
        o[:len(self.const)] = self.const
        return o


def expect(s):
    """(segs, acks, opts, count) whole, guards included, and the model's own four outputs."""
    segs, acks, count, blocks = s.model()
    cap = s.args["cap"]
    wsegs = np.full((cap + GUARD) * 32, FILL, np.uint8).view(rxg.TX_SEG_DTYPE)
    wacks = np.full((cap + GUARD) * 16, FILL, np.uint8).view(rxg.ACK_DTYPE)
    wsegs[:len(segs)] = segs
    wacks[:len(acks)] = acks
    wopts = s.opts_in()
    for k, b in blocks.items():
        assert len(s.const) <= k < s.args["opt_cap"]
        wopts[k] = b
    return (wsegs, wacks, wopts, count), (segs, acks, count, blocks)


def states(nflows, seed):
    rng = np.random.default_rng(seed)
    st = np.zeros(nflows, dtype=rxg.ACK_STATE_DTYPE)
    st["snd_nxt"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    st["rcv_ack"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    st["ts_recent"] = rng.integers(0, 1 << 32, nflows, dtype=np.uint64)
    st["win_raw"] = 12000
    f = np.arange(nflows)
    st["flags"] = np.where(f % 7 == 3, 0, LIVE) | np.where(f % 3 == 1, TS, 0)
    return st


def ts_records(n, with_ts=True):
    r = np.zeros(n, dtype=rxg.RX_OPT_DTYPE)
    r["flags"] = rxg.O_PARSED | (rxg.O_TS if with_ts else rxg.O_MSS)
    r["tsval"] = 5000 + np.arange(n)          # (set also without O_TS: it must not be echoed then)
    r["tsecr"] = 77
    r["opt_len"] = 12
    return r


def flow_lengths(T, shape):
    """The flows' train counts for T trains.  `mixed`: 1-5 trains, bent so that in every even tile a
    flow ends at the tile's edge (the next flow's first train is lane 0) and a flow that begins on
    lane 255 has at least two trains (it straddles the edge)."""
    if shape == "own":
        return [1] * T
    if shape == "one":
        return [T]
    out, k, j = [], 0, 0
    while k < T:
        ln = 1 + (j * 7 + j // 5) % 5
        j += 1
        lane, tile = k % TILE, k // TILE
        if lane + ln > TILE and lane != TILE - 1 and tile % 2 == 0:
            ln = TILE - lane
        if lane == TILE - 1:
            ln = max(ln, 2)
        ln = min(ln, T - k)
        out.append(ln)
        k += ln
    return out


def shaped(T, shape):
    lens = flow_lengths(T, shape)
    nflows = len(lens)
    tcb = np.repeat(np.arange(nflows), lens)
    firsts = np.cumsum([0] + lens[:-1])
    flags = np.zeros(T, dtype=np.uint32)
    f = np.arange(nflows)
    flags[firsts] = FIRST | np.where(f % 2 == 0, HEAD, 0) | np.where(f % 5 == 2, FIN, 0)
    flags[firsts + np.array(lens) - 1] |= LAST
    later = np.ones(T, bool)
    later[firsts] = False
    flags[later] |= np.where(np.arange(T)[later] % 3 == 0, FIN, 0).astype(np.uint32)   # later trains' flags must not matter
    next_ack = (np.arange(T, dtype=np.uint64) * 2654435761 + 17) & 0xFFFFFFFF
    return Set(f"T={T} {shape}", tcb, flags, next_ack, states(nflows, T), nflows, rxopts=ts_records(T),
               ip_id0=0xFFF0)


SIZES = [1, 63, 64, 65, 255, 256, 257, ROUND + 1]


def size_sets():
    return [shaped(T, shape) for T in SIZES for shape in ("own", "mixed", "one")]


def combo_sets():
    """{LIVE or not} x {HEAD or not} x {FIN or not} x {TS or not} on 16 neighbouring lanes, with
    rxopts NULL, given with RXG_O_TS and given without."""
    st = states(16, 99)
    flags = np.zeros(16, dtype=np.uint32)
    for f in range(16):
        st["flags"][f] = (LIVE if f & 1 else 0) | (TS if f & 8 else 0)
        flags[f] = FIRST | LAST | (HEAD if f & 2 else 0) | (FIN if f & 4 else 0)
    # trains of two segments, so that a train's first and last segment are different packets
    base = Set("combos", np.arange(16), flags, 70000 + np.arange(16), st, 16, order=np.arange(32)[::-1].copy(),
               first=2 * np.arange(16), nseg=2, n=32)
    return [base.variant("rxopts NULL", rxopts=None), base.variant("rxopts TS", rxopts=ts_records(32)),
            base.variant("rxopts no TS", rxopts=ts_records(32, False)),
            base.variant("opts NULL", rxopts=ts_records(32), use_opts=False)]


def range_set():
    ntcb = 9
    tcb = [-1, 0, 3, 3, ntcb - 1, ntcb, ntcb + 1, 0x7FFFFFFF]
    st = states(ntcb, 5)
    st["flags"] = LIVE | TS
    return Set("tcb_idx -1, ntcb - 1, ntcb, 0x7FFFFFFF", tcb, [FIRST | HEAD] * len(tcb), 100 + np.arange(len(tcb)), st, ntcb,
               rxopts=ts_records(len(tcb)))


def wrap_set():
    st = states(40, 11)
    st["flags"] = LIVE
    st["flags"][::2] |= TS
    return Set("ip_id0 0xFFF0 over 40 ACKs", np.arange(40), [FIRST | HEAD] * 40, 9 + np.arange(40), st, 40, ip_id0=0xFFF0,
               opt_base=2, opt_plain=1)


def cap_sets():
    base = wrap_set()
    need = 40
    out = [base.variant(f"cap {c}", cap=c) for c in (0, need - 1, need, need + 3)]
    # opt_cap at opt_base, opt_base + 1, one below and at the need (the last TS flow is ACK 38)
    out += [base.variant(f"opt_cap {c}", opt_cap=c) for c in (2, 3, 2 + 38, 2 + 39)]
    out += [base.variant("opt_plain 0", opt_plain=0), base.variant("opt_plain 1, cap 5, opt_cap 4", cap=5, opt_cap=4)]
    return out


def extreme_set():
    vals = [0, 0xFFFFFFFF, 0x80000000]
    st = np.zeros(9, dtype=rxg.ACK_STATE_DTYPE)
    tcb, flags, nack = [], [], []
    for f in range(9):
        st[f] = (vals[f % 3], vals[f // 3], vals[(f + 1) % 3], 0xFFFF if f % 2 else 0, LIVE | TS)
        tcb.append(f)
        flags.append(FIRST | (HEAD if f >= 3 else 0) | (FIN if f == 4 else 0))
        nack.append(vals[(f + 2) % 3])
    return Set("snd_nxt, rcv_ack, next_ack at 0, 2^32 - 1, 2^31", tcb, flags, nack, st, 9, rxopts=ts_records(9),
               tsval_now=0xFFFFFFFF, ip_id0=0xFFFF)


def count_sets():
    base = shaped(300, "mixed")
    return [base.variant("count[1] 257 < cap_trains", train_count=np.array([300, 257, 0, 0], np.uint64)),
            base.variant("cap_trains 256 < count[1]", cap_trains=256),
            base.variant("count[1] 2^40", train_count=np.array([300, 1 << 40, 0, 0], np.uint64)),
            base.variant("n 255 < count[1]", n=255, rxopts=ts_records(255)),
            base.variant("cap_seg 10 (firsts past S')", cap_seg=10),
            base.variant("T' 0: count[1] 0", train_count=np.array([300, 0, 0, 0], np.uint64)),
            base.variant("T' 0: count[0] 0", train_count=np.array([0, 300, 0, 0], np.uint64)),
            base.variant("T' 0: cap_trains 0", cap_trains=0),
            base.variant("n 0", n=0, rxopts=None)]


def flow_first_set():
    """RXG_FTR_FLOW_FIRST wrong on purpose: set on a later train, missing on the first."""
    tcb = [0, 0, 0, 1, 2, 2]
    flags = [HEAD, FIRST, FIRST | HEAD, 0, FIRST, FIRST]
    st = states(3, 2)
    st["flags"] = LIVE | TS
    return Set("FLOW_FIRST on a later train, missing on the first", tcb, flags, [10, 20, 30, 40, 50, 60], st, 3,
               rxopts=ts_records(6))


def order_set():
    """order[first] >= n, and first >= S': ts_recent is echoed, rxopts never indexed."""
    st = states(5, 8)
    st["flags"] = LIVE | TS
    return Set("order[first] >= n", np.arange(5), [FIRST | HEAD] * 5, 10 * np.arange(5), st, 5,
               order=[2, 5, 0xFFFFFFFF, 1, 4, 9, 9], first=[0, 1, 2, 3, 5], n=5, rxopts=ts_records(5), cap_seg=5)


def small_sets():
    return (combo_sets() + [range_set(), wrap_set()] + cap_sets() + [extreme_set()] + count_sets() +
            [flow_first_set(), order_set()])


def all_sets():
    return size_sets() + small_sets()
