"""Scripts and their expected answers for what a replay hands out (csrc/rxg_attached.h), for
tests/test_attached_host.py: each set is a list of the commands tests/attached_check.cpp plays over
the real rxg::ReplayAttached and rxg::RcvWindow, and Model.run says what every take must answer.

The model is written from the contracts of include/rxg.h (rxg_reset_take, rxg_rx_opt_current,
rxg_flow_sum_current, rxg_flow_train_current, rxg_ack_take, rxg_rcv_set, rxg_payload_take), never
from the C++: a reset is looked up by its packet (no cursor), a train by scanning every train's
segments (no binary search), an ACK by listing every condition that refuses it.  The summaries,
trains and ACKs that get attached are those of flowsum_ref, flowtrain_ref and ackplan_ref.  While it
answers, the model notes which edge each answer went through (Model.hits); every set names the edges
it is there for and build() asserts that its script reached them."""
import numpy as np

import ackplan_ref
import flowsum_cases as fc
import flowsum_ref
import flowtrain_cases as ftc
import flowtrain_ref
import pktgen
import rxg

M32 = 0xFFFFFFFF
DISPATCH, NOPCB, DROP = rxg.V_DISPATCH, rxg.V_RST_NOPCB, rxg.V_DROP_NONTCP
DST = pktgen.raw_of_host(fc.DST)
NTCB = 8            # the plans' and the mirror's table: slots 0 .. 6 live, 7 never written


def key(i):
    """The tuple of slot i as the mirror keys it: (dport << 16 | sport, dst, src)."""
    return ((80 << 16) | (2000 + i), DST, fc.flow_src(i))


def tcb(i, variant=0):
    return ("tcb", i, 80, 2000 + i + 100 * variant, DST, fc.flow_src(i))


def table():
    return [tcb(i) for i in range(NTCB - 1)]


def reset_frame(k, ip_id):
    """The 64 bytes attached_check.cpp builds for slot k: a pattern, the id stored as it stands at
    18..19, and the IPv4 header checksum over bytes 14..34 (rxg.h: rxg_reset_set_id)."""
    f = bytearray((17 * k + 3 * b + 1) & 0xFF for b in range(64))
    return with_id(f, ip_id)


def with_id(f, ip_id):
    f = bytearray(f)
    f[18], f[19] = ip_id & 0xFF, ip_id >> 8
    f[24:26] = b"\0\0"
    f[24:26] = pktgen.py_checksum(bytes(f[14:34])).to_bytes(2, "big")
    return f


class Model:
    def __init__(self):
        self.slot = {}                       # live slots: idx -> key
        self.touched_all, self.touched_keys = False, set()
        self.burst = []                      # the records as the burst wrote them: (verdict, tcb)
        self.pos = self.n = None             # the running replay's packet and size
        self.fixed = {}                      # packets the running replay re-classified -> new record
        self.seen_at = False
        self.resets = self.opts = self.sums = self.trains = None
        self.rst_last = None
        self.acks, self.ak_live, self.ak_ever = None, False, False
        self.void_all, self.void_keys, self.void_tcb = None, {}, {}
        self.rcv = []                        # [cur, state] per slot; state "unknown" / "none" / "pairs"
        self.hits = set()
        self.out = []

    def run(self, script):
        for c in script:
            getattr(self, "do_" + c[0])(*c[1:])
        return self.out

    # ------------------------------------------------------------- the context's part ---
    def do_tcb(self, idx, dport, sport, dst, src):
        self.slot[idx] = ((dport << 16) | sport, dst, src)

    def do_tcbrm(self, idx):
        self.slot.pop(idx, None)

    def do_touch(self, what, *k):
        if what == "all":
            self.touched_all = True
        elif what == "clear":
            self.touched_all, self.touched_keys = False, set()
        else:
            self.touched_keys.add(tuple(k))

    def do_recs(self, n, *flat):
        self.burst = [(flat[2 * i], flat[2 * i + 1]) for i in range(n)]

    # ---------------------------------------------------------------- the attachments ---
    def do_resets(self, n, *flat):
        self.resets = [(flat[2 * k], reset_frame(k, flat[2 * k + 1])) for k in range(n)]
        self.rst_last = None

    def do_opts(self, n):
        self.opts = n

    def do_sums(self, m, *flat):
        rows = [tuple(flat[3 * k:3 * k + 3]) for k in range(m)]
        for k in range(1, m):
            if rows[k][0] <= rows[k - 1][0]:       # rxg.h: entries strictly ascending in tcb_idx
                self.out.append("sums bad %d" % k)
                self.hits.add("sum:attach_refused")
                return
        self.sums = rows
        self.out.append("sums ok")

    def do_trains(self, nseg, *flat):
        order, nt = list(flat[:nseg]), flat[nseg]
        rows = [tuple(flat[nseg + 1 + 3 * k:nseg + 4 + 3 * k]) for k in range(nt)]
        at = 0
        for k, (t, first, ns) in enumerate(rows):  # rxg.h: train k starts where k - 1 ended, nseg >= 1, tcb_idx never descending
            why = "gap" if first != at else "nseg0" if ns == 0 else "descends" if k and t < rows[k - 1][0] else None
            if why:
                self.out.append("trains bad %d %d" % (k, at))
                self.hits.add("train:attach_" + why)
                return
            at += ns
        self.trains = (order, rows)
        self.out.append("trains ok")

    def do_acks(self, n, stride, *flat):
        rows = [tuple(flat[3 * k:3 * k + 3]) for k in range(n)]   # (tcb, seq, ack)
        for a in range(1, n):
            if rows[a][0] <= rows[a - 1][0]:
                self.out.append("acks bad %d" % a)
                self.hits.add("ack:attach_refused")
                return
        if self.acks is not None:
            self.hits.add("ack:reattach")
        self.acks, self.ak_live = (rows if n else None), False
        self.ak_ever = self.ak_ever or n > 0
        self.void_all, self.void_keys, self.void_tcb = None, {}, {}
        self.out.append("acks ok")

    # --------------------------------------------------------------------- the replay ---
    def ack_step(self):
        """rxg.h: the attachment outlives its own replay and ends at the rxg_rx_replay after it."""
        if self.ak_live:
            self.acks, self.ak_live = None, False
            self.hits.add("ack:second_replay_ends")
        elif self.acks is not None:
            self.ak_live = True

    def do_begin(self, n):
        assert n == len(self.burst)
        self.ack_step()
        self.n, self.pos, self.fixed, self.seen_at = n, None, {}, False

    def do_beginfail(self, n):
        self.ack_step()
        self.n = n
        if self.acks is not None:
            self.hits.add("ack:failed_replay_ends")
        self.do_end(0)

    def do_absorb(self, all_, nk, *flat):
        if self.ak_live:
            where = "handler" if self.seen_at else "launch"
            if all_:
                self.void_all = where
            for k in range(nk):
                self.void_keys.setdefault(tuple(flat[3 * k:3 * k + 3]), where)

    def do_fix(self, j, verdict, t):
        old = self.fixed.get(j, self.burst[j])
        if self.ak_live:
            self.void_tcb.setdefault(old[1], "old")
            self.void_tcb.setdefault(t, "new")
        self.fixed[j] = (verdict, t)

    def do_at(self, i):
        self.pos, self.seen_at = i, True

    def do_end(self, ran):
        self.pos = self.n = None
        self.resets = self.opts = self.sums = self.trains = None
        if not ran:
            self.acks, self.ak_live = None, False

    # ---------------------------------------------------------------------- the takes ---
    def refuse(self, what, why):
        self.hits.add(what + ":" + why)
        self.out.append(what + " -1")

    def do_reset(self, ip_id):
        if self.pos is None:
            return self.refuse("reset", "outside")
        if self.resets is None:
            return self.refuse("reset", "nothing")
        if not self.resets:
            return self.refuse("reset", "nbuilt0")
        ks = [k for k, (p, _) in enumerate(self.resets) if p == self.pos]
        if not ks:
            return self.refuse("reset", "none_for_packet")
        k, = ks
        f = self.resets[k][1]
        if (f[18] | (f[19] << 8)) == ip_id:
            self.hits.add("reset:same_id")
        else:
            f[:] = with_id(f, ip_id)
            self.hits.add("reset:rewritten")
        if self.rst_last is not None and k > self.rst_last + 1:
            self.hits.add("reset:skipped")
        if self.rst_last is not None and k == self.rst_last + 1 and self.resets[k - 1][0] == self.pos - 1:
            self.hits.add("reset:consecutive")
        if self.rst_last == k:
            self.hits.add("reset:again")
        self.rst_last = k
        self.out.append("reset %d %s" % (k, f.hex()))

    def do_opt(self):
        if self.pos is None:
            return self.refuse("opt", "outside")
        if not self.opts:
            return self.refuse("opt", "nothing")
        if self.opts != self.n:
            return self.refuse("opt", "n_differs")
        self.hits.add("opt:reclassified" if self.pos in self.fixed else "opt:answered")
        self.out.append("opt %d" % self.pos)

    def burst_dispatch(self, what):
        """The TCB of the packet's record as the burst wrote it, if a DISPATCH the replay kept."""
        if self.pos in self.fixed:
            return self.refuse(what, "reclassified")
        v, t = self.burst[self.pos]
        if v != DISPATCH:
            return self.refuse(what, "not_dispatch")
        return t

    def do_sum(self):
        if self.pos is None:
            return self.refuse("sum", "outside")
        if not self.sums:
            return self.refuse("sum", "nothing")
        t = self.burst_dispatch("sum")
        if t is None:
            return
        ks = [k for k, r in enumerate(self.sums) if r[0] == t]
        if not ks:
            return self.refuse("sum", "flow_absent")
        _, first, last = self.sums[ks[0]]
        if self.pos < first:
            return self.refuse("sum", "below_first")
        if self.pos > last:
            return self.refuse("sum", "above_last")
        self.hits.add("sum:answered")
        self.out.append("sum %d %d" % (ks[0], self.pos))

    def do_train(self):
        if self.pos is None:
            return self.refuse("train", "outside")
        if not self.trains or not self.trains[0] or not self.trains[1]:
            return self.refuse("train", "nothing")
        t = self.burst_dispatch("train")
        if t is None:
            return
        order, rows = self.trains
        mine = [k for k, r in enumerate(rows) if r[0] == t]
        if not mine:
            return self.refuse("train", "flow_absent")
        for k in mine:
            _, first, ns = rows[k]
            segs = order[first:first + ns]          # what of the train the attached order holds
            if self.pos in segs:
                if first + ns > len(order):
                    return self.refuse("train", "order_capped")
                p = segs.index(self.pos)
                if ns >= 3:
                    self.hits.add("train:%s_of_%d" % ("first" if p == 0 else "last" if p == ns - 1 else "middle",
                                                      mine.index(k)))
                if len(mine) >= 3:
                    self.hits.add("train:three_trains")
                self.out.append("train %d %d" % (k, p))
                return
        if self.pos in order:
            return self.refuse("train", "trains_capped")
        self.refuse("train", "no_segment")

    def do_ack(self, t, snd_nxt, rcv_ack):
        if not self.ak_live:
            return self.refuse("ack", "before_replay" if self.acks is not None else
                               "detached" if self.ak_ever else "before_attach")
        if t < 0:                                  # names no TCB
            return self.refuse("ack", "negative")
        no = []
        rows = [(a, r) for a, r in enumerate(self.acks) if r[0] == t]
        if not rows:
            no.append("no_entry")
        else:
            if rows[0][1][1] != snd_nxt:
                no.append("seq_off_by_%d" % abs(rows[0][1][1] - snd_nxt))
            if rows[0][1][2] != rcv_ack:
                no.append("ack_off_by_%d" % abs(rows[0][1][2] - rcv_ack))
        if t not in self.slot:
            no.append("not_live" if t <= max(self.slot, default=-1) else "past_ntcb")
        else:
            k = self.slot[t]
            if k in self.void_keys:
                no.append("written_" + self.void_keys[k])
            if k in self.touched_keys:
                no.append("touched")
        if t in self.void_tcb:
            no.append("reclassified_" + self.void_tcb[t])
        if self.void_all:
            no.append("all_" + self.void_all)
        if self.touched_all:
            no.append("touched_all")
        if no:
            if len(no) == 1:                       # refused by this alone
                self.hits.add("ack:" + no[0])
            self.out.append("ack -1")
            return
        self.hits.add("ack:answered_in_replay" if self.pos is not None else "ack:answered_after_replay")
        if self.void_keys or self.void_tcb or self.touched_keys:
            self.hits.add("ack:untouched_beside_voided")
        self.out.append("ack %d" % rows[0][0])

    # ------------------------------------------------------------- the receive window ---
    def do_rcvset(self, idx, cur, pairs):
        if idx >= len(self.rcv):
            self.hits.add("rcv:grown")
            self.rcv += [[0, "unknown"] for _ in range(idx + 1 - len(self.rcv))]
        self.rcv[idx] = [cur, "pairs" if pairs else "none"]
        self.out.append("rcvsize %d" % len(self.rcv))

    def do_rcvforget(self, idx):
        if idx < len(self.rcv):
            self.rcv[idx][1] = "unknown"

    def do_rcvclear(self):
        self.rcv = []

    def do_pay(self, idx, seq, length, mflags, mlen):
        """rxg.h rxg_payload_take; seq 0: GetData asserts CurrentSequenceNumber != 0 (tcp_windows.c:151)."""
        no = []
        if not mflags & rxg.PM_GATHERED:
            no.append("not_gathered")
        if mlen != length:
            no.append("other_length")
        if not 0 <= idx < len(self.rcv):
            no.append("index")
        else:
            cur, state = self.rcv[idx]
            if state != "none":
                no.append("window_" + state)
            if cur != seq:
                no.append("cur_differs")
        if seq > ((seq + length) & M32):
            no.append("duplicate_test")
        if seq == 0:
            no.append("seq_zero")
        if len(no) == 1:
            self.hits.add("pay:" + no[0])
        if not no:
            self.rcv[idx][0] = (seq + length) & M32
            self.hits.add("pay:taken")
        self.out.append("pay %d" % (0 if no else 1))


# ------------------------------------------------------------------------------- sets ---
def recs_cmd(pairs):
    return ("recs", len(pairs)) + tuple(int(x) for p in pairs for x in p)


def resets_set():
    rst = {1: 100, 3: 101, 4: 102, 6: 103, 8: 104}
    burst = [(NOPCB, -1) if i in rst else (DISPATCH, 0) for i in range(10)]
    s = [recs_cmd(burst), ("resets", len(rst)) + tuple(x for p in sorted(rst.items()) for x in p), ("reset", 100),
         ("begin", 10), ("at", 0), ("reset", 100),
         ("at", 1), ("reset", 100), ("reset", 100),      # the id it was built with, twice
         ("at", 3), ("reset", 101), ("at", 4), ("reset", 0xBEEF),   # consecutive; another id
         ("at", 5), ("reset", 5),
         ("at", 8), ("reset", 0x0102),                   # packet 6's was never taken: passed over
         ("at", 9), ("reset", 9), ("end", 1), ("reset", 100),
         ("begin", 10), ("at", 1), ("reset", 100), ("end", 1),      # the attachment ended with its replay
         ("resets", 0), ("begin", 10), ("at", 1), ("reset", 100), ("end", 1)]
    return s, {"reset:outside", "reset:none_for_packet", "reset:same_id", "reset:again", "reset:consecutive",
               "reset:rewritten", "reset:skipped", "reset:nothing", "reset:nbuilt0"}


def opts_set():
    burst = [(DISPATCH, i % 3) for i in range(6)]
    s = table() + [recs_cmd(burst), ("opts", 6), ("opt",), ("begin", 6), ("at", 0), ("opt",), ("at", 2), ("opt",),
                   ("absorb", 0, 1) + key(0), ("fix", 3, NOPCB, -1), ("at", 3), ("opt",), ("at", 5), ("opt",),
                   ("end", 1), ("opt",), ("begin", 6), ("at", 0), ("opt",), ("end", 1),
                   ("opts", 5), ("begin", 6), ("at", 0), ("opt",), ("at", 4), ("opt",), ("end", 1)]
    return s, {"opt:outside", "opt:answered", "opt:reclassified", "opt:nothing", "opt:n_differs"}


def sums_of(rec48, ntcb=NTCB):
    out, _ = flowsum_ref.summaries(rec48, rxg.REC48, ntcb)
    return [(int(r["tcb_idx"]), int(r["first_idx"]), int(r["last_idx"])) for r in out]


def sums_cmd(rows):
    return ("sums", len(rows)) + tuple(x for r in rows for x in r)


def sums_set():
    tcbs = [0, 1, 0, 2, 1, 3, 0, 2, 1, 0, 4, 1]
    rec = fc.craft(tcbs, seq=np.arange(12) + 1, ack=1)
    c = rec["c"]
    c["verdict"][5] = NOPCB                              # a record that is no DISPATCH
    rec["c"] = c
    burst = [(int(v), int(t)) for v, t in zip(rec["c"]["verdict"], rec["c"]["tcb_idx"])]
    whole = sums_of(rec)
    inner = rec.copy()                                   # another call's list: only packets 2 .. 8 counted
    ci = inner["c"]
    ci["verdict"][[0, 1, 9, 10, 11]] = DROP
    inner["c"] = ci
    narrow = sums_of(inner)
    everyone = [x for i in range(12) for x in (("at", i), ("sum",))]
    s = table() + [recs_cmd(burst), sums_cmd(whole), ("sum",), ("begin", 12)] + everyone[:8]
    s += [("absorb", 0, 1) + key(1), ("fix", 4, NOPCB, -1)] + everyone[8:] + [("end", 1), ("sum",)]
    s += [sums_cmd(whole[:2]), ("begin", 12)] + everyone + [("end", 1)]     # capped: flows past cap are absent
    s += [sums_cmd(narrow), ("begin", 12)] + everyone + [("end", 1)]
    s += [sums_cmd(whole), sums_cmd(whole[:2] + [whole[3], whole[2]]), ("begin", 12), ("at", 0), ("sum",), ("end", 1)]
    s += [("begin", 12), ("at", 0), ("sum",), ("end", 1)]
    assert [r[0] for r in whole] == [0, 1, 2, 4] and narrow != whole
    return s, {"sum:outside", "sum:answered", "sum:not_dispatch", "sum:reclassified", "sum:flow_absent",
               "sum:below_first", "sum:above_last", "sum:attach_refused", "sum:nothing"}


def trains_of(rec48, ntcb=NTCB, cur_seq=None):
    order, t, _ = flowtrain_ref.trains(rec48, rxg.REC48, ntcb, cur_seq=cur_seq)
    return [int(x) for x in order], t


def trains_cmd(order, rows):
    return ("trains", len(order)) + tuple(order) + (len(rows),) + tuple(x for r in rows for x in r)


def train_rows(t):
    return [(int(r["tcb_idx"]), int(r["first"]), int(r["nseg"])) for r in t]


def trains_burst():
    """Flow 1: three trains of three segments and one ACK without data; flows 0 and 2 between them;
    one RST."""
    parts = {0: ftc.chain(0, 500, [10, 10]), 2: ftc.chain(2, 900, [7, 7, 7]),
             1: ftc.cat(ftc.chain(1, 1000, [5, 5, 5]), ftc.chain(1, 5000, [5, 5, 5]), ftc.chain(1, 9000, [5, 5, 5]))}
    flow_of = [1, 0, 1, 2, 1, 1, 9, 1, 2, 1, 0, 1, 8, 1, 2, 1]      # 9: flow 1's ACK without data, 8: the RST
    nxt = {0: 0, 1: 0, 2: 0}
    rows = []
    for f in flow_of:
        if f == 9:
            rows.append(ftc.craft([1], [1015], [0]))
        elif f == 8:
            rows.append(ftc.craft([-1], [1], [4], verdict=NOPCB))
        else:
            rows.append(parts[f][nxt[f]:nxt[f] + 1])
            nxt[f] += 1
    return np.concatenate(rows)


def trains_set():
    rec = trains_burst()
    n = len(rec)
    burst = [(int(v), int(t)) for v, t in zip(rec["c"]["verdict"], rec["c"]["tcb_idx"])]
    order, t = trains_of(rec)
    rows = train_rows(t)
    assert [r[0] for r in rows] == [0, 1, 1, 1, 2] and all(r[2] == 3 for r in rows[1:4]) and len(order) == 14
    everyone = [x for i in range(n) for x in (("at", i), ("train",))]
    cut = rows[2][1] + 1                                 # order capped inside flow 1's second train
    s = table() + [recs_cmd(burst), trains_cmd(order, rows), ("train",), ("begin", n)] + everyone[:16]
    s += [("absorb", 0, 1) + key(1), ("fix", 9, NOPCB, -1)] + everyone[16:] + [("end", 1), ("train",)]
    s += [trains_cmd(order[:cut], rows), ("begin", n)] + everyone + [("end", 1)]
    s += [trains_cmd(order, rows[:3]), ("begin", n)] + everyone + [("end", 1)]
    s += [trains_cmd(order, rows[1:]),                                         # train 0 does not start at 0
          trains_cmd(order, rows[:2] + [(1, rows[2][1], 0)] + rows[3:]),
          trains_cmd(order, [(3,) + rows[0][1:]] + rows[1:]),
          trains_cmd(order, rows[:2] + [(1, rows[2][1] + 1, 2)] + rows[3:]),   # a gap inside
          ("begin", n), ("at", 0), ("train",), ("end", 1)]
    hits = {"train:outside", "train:three_trains", "train:no_segment", "train:not_dispatch", "train:reclassified",
            "train:order_capped", "train:trains_capped", "train:flow_absent", "train:nothing", "train:attach_gap",
            "train:attach_nseg0", "train:attach_descends"}
    hits |= {"train:%s_of_%d" % (w, k) for w in ("first", "middle", "last") for k in range(3)}
    return s, hits


def acks_of(rec48, state, cur_seq):
    """The ACKs ackplan_ref plans for the burst's trains: rows (tcb, seq, ack)."""
    order, t = trains_of(rec48, cur_seq=cur_seq)
    count = np.array([len(order), len(t), 0, 0], np.uint64)
    _, acks, _, _ = ackplan_ref.plan(np.array(order, np.uint32), t, count, len(rec48), NTCB, state)
    return [(int(a["tcb_idx"]), int(a["seq"]), int(a["ack"])) for a in acks]


def acks_cmd(rows, stride=64):
    return ("acks", len(rows), stride) + tuple(x for r in rows for x in r)


def acks_plan():
    """One data segment on each flow 0 .. 7 (slot 7 is in the plan's table, never in the mirror)."""
    rec = ftc.cat(*[ftc.chain(f, 1000 * (f + 1), [100]) for f in range(NTCB)])
    state = np.zeros(NTCB, dtype=rxg.ACK_STATE_DTYPE)
    state["snd_nxt"], state["rcv_ack"], state["win_raw"], state["flags"] = 7000 + np.arange(NTCB), 50, 1000, rxg.AS_LIVE
    cur = np.zeros(NTCB, np.uint32)
    cur[::2] = 1000 * (np.arange(NTCB)[::2] + 1)         # even flows: HEAD trains, their ACK advances
    rows = acks_of(rec, state, cur)
    assert [r[0] for r in rows] == list(range(NTCB)) and rows[0][2] == 1100 and rows[1][2] == 50
    burst = [(DISPATCH, f) for f in range(NTCB)]
    return burst, rows


def ask(rows, tcbs):
    return [("ack",) + rows[t] for t in tcbs]


def acks_phase_set():
    burst, rows = acks_plan()
    n = len(burst)
    s = table() + [recs_cmd(burst)] + ask(rows, [0]) + [acks_cmd(rows)] + ask(rows, [0, 1])
    s += [("begin", n), ("at", 0)] + ask(rows, [0, 3]) + [("at", 5)] + ask(rows, [5]) + [("end", 1)] + ask(rows, [0, 6])
    s += [("begin", n), ("at", 0)] + ask(rows, [0]) + [("end", 1)] + ask(rows, [0])       # a second replay ended it
    s += [acks_cmd(rows), ("beginfail", n)] + ask(rows, [0])                              # a refused one too
    s += [acks_cmd(rows), ("begin", n), ("end", 0)] + ask(rows, [0])                      # and one that failed later
    s += [acks_cmd(rows), acks_cmd(rows[:3], 128), ("begin", n), ("at", 1)] + ask(rows, [2, 3]) + [("end", 1)]
    s += ask(rows, [1]) + [acks_cmd([rows[1], rows[0]] + rows[2:])] + ask(rows, [1]) + [("acks", 0, 0)] + ask(rows, [1])
    return s, {"ack:before_attach", "ack:before_replay", "ack:answered_in_replay", "ack:answered_after_replay",
               "ack:second_replay_ends", "ack:failed_replay_ends", "ack:detached", "ack:reattach", "ack:no_entry",
               "ack:attach_refused"}


def acks_void_set():
    burst, rows = acks_plan()
    n = len(burst)
    off = lambda r, ds, da: ("ack", r[0], (r[1] + ds) & M32, (r[2] + da) & M32)
    s = table() + [recs_cmd(burst), acks_cmd(rows), ("touch", "key") + key(6), ("begin", n)]
    s += [("absorb", 0, 1) + key(6), ("touch", "clear"), ("at", 0)] + ask(rows, [6, 0])   # absorbed at the start
    s += [("absorb", 0, 1) + key(1), ("fix", 2, DISPATCH, 3), ("at", 2)]    # packet 2 moves from TCB 2 to TCB 3
    s += ask(rows, [1, 2, 3, 0])
    s += [off(rows[0], 1, 0), off(rows[0], -1, 0), off(rows[0], 0, 1), off(rows[0], 0, -1)]
    s += [("ack", -1, rows[0][1], rows[0][2]), ("ack", 7, rows[7][1], rows[7][2]), ("ack", 9, 1, 1)]
    s += [("at", 7), ("end", 1)] + ask(rows, [4, 5])
    s += [("tcbrm", 4)] + ask(rows, [4, 5])                                 # a slot no longer live
    s += [tcb(5, 1), ("touch", "key") + key(5), ("touch", "key", (80 << 16) | 2105, DST, fc.flow_src(5))]   # after the replay
    s += ask(rows, [5, 0]) + [("touch", "all")] + ask(rows, [0]) + [("touch", "clear")]
    s += [acks_cmd(rows), ("begin", n), ("at", 0)] + ask(rows, [0]) + [("absorb", 1, 0)] + ask(rows, [0]) + [("end", 1)]
    s += ask(rows, [0])
    return s, {"ack:written_launch", "ack:written_handler", "ack:reclassified_old", "ack:reclassified_new",
               "ack:seq_off_by_1", "ack:ack_off_by_1", "ack:negative", "ack:past_ntcb", "ack:not_live",
               "ack:touched", "ack:touched_all", "ack:all_handler", "ack:untouched_beside_voided",
               "ack:answered_in_replay", "ack:answered_after_replay"}


def window_set():
    G = rxg.PM_GATHERED
    s = [("pay", 0, 100, 10, G, 10), ("rcvset", 2, 100, 0), ("rcvset", 1, 300, 1), ("rcvset", 5, 0, 0),
         ("pay", 2, 100, 10, 0, 10),                                # flags
         ("pay", 2, 100, 10, G, 11),                                # length
         ("pay", 6, 100, 10, G, 10), ("pay", -1, 100, 10, G, 10),   # index
         ("pay", 0, 0, 10, G, 10),                                  # a slot never set (its cur 0 = seq: seq 0 too)
         ("pay", 1, 300, 10, G, 10),                                # pairs pending
         ("pay", 2, 101, 10, G, 10),                                # cur
         ("rcvset", 3, 0xFFFFFFFE, 0), ("pay", 3, 0xFFFFFFFE, 10, G, 10),   # the duplicate test: seq + Length wraps
         ("pay", 5, 0, 10, G, 10),                                  # seq 0
         ("pay", 2, 100, 10, G, 10), ("pay", 2, 100, 10, G, 10),    # taken; the same segment again
         ("pay", 2, 110, 1000, G | rxg.PM_REF_OVERSIZE, 1000), ("rcvset", 3, 0xFFFFFFF6, 0),
         ("pay", 3, 0xFFFFFFF6, 9, G, 9), ("pay", 3, 0xFFFFFFFF, 1, G, 1),   # up to 2^32 - 1; the next would wrap
         ("rcvforget", 2), ("pay", 2, 1110, 10, G, 10), ("rcvforget", 9), ("rcvset", 2, 1110, 0), ("pay", 2, 1110, 10, G, 10),
         ("rcvclear",), ("pay", 2, 1120, 10, G, 10), ("rcvset", 0, 7, 0), ("pay", 0, 7, 3, G, 3)]
    return s, {"rcv:grown", "pay:not_gathered", "pay:other_length", "pay:index", "pay:window_pairs",
               "pay:window_unknown", "pay:cur_differs", "pay:duplicate_test", "pay:seq_zero", "pay:taken"}


SETS = {"resets": resets_set, "options": opts_set, "flow sums": sums_set, "flow trains": trains_set,
        "acks phases": acks_phase_set, "acks voiding": acks_void_set, "receive window": window_set}
ALL = list(SETS)
MAX_PACKETS = 64


def build(name):
    """(the script's text, the answers it must print), after asserting that the set is small and
    that its script reaches every edge it is named for."""
    script, edges = SETS[name]()
    m = Model()
    want = m.run(script)
    assert edges <= m.hits, (name, sorted(edges - m.hits))
    assert all(c[1] <= MAX_PACKETS for c in script if c[0] in ("recs", "begin", "beginfail"))
    return "".join(" ".join(str(int(x)) if not isinstance(x, str) else x for x in c) + "\n" for c in script), want
