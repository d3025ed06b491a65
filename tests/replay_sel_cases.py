"""Deterministic edge sets for the replay's selected re-classification (rxg_rx_replay's reclassify():
rx_kernel<16, kDescSel, false, false>, csrc/rxg_replay.cpp and rxg_rx.h load_desc), the epoch
expectation, and a model of the selection.

Frames that name themselves.  TABLE holds F = 257 ESTABLISHED flows on dport 80 and listeners on 80
and 8080 in the row shape of test_gpu_replay.scenario, behind two spare ESTABLISHED rows whose
tuples no frame carries and one NULL slot (the `minnull` writer needs a live row below the lowest
NULL slot, and below the port-80 listener so that REF_NULLSLOT of a pass-2 packet moves with it):

    0, 1 spare   2 LISTENING :80   3 NULL   4 .. 260 flow 0 .. 256   261 LISTENING :8080

Frame i of a case carries the tuple of flow i mod 257 (64 and 257 are coprime: the 64 frames of a
list slice, and a slice's neighbours, all differ), so a record taken from another frame shows a
wrong tcb_idx.  Pass-2 packets come from client i mod 60, whom no row names.

Writers.  A writer is a flow frame whose tcpswitch handler makes one write (apply_writer, on the
python rows and, with an engine, through rxg_tcb_*): `reload` loads the table rotated by one slot
(every index moves; touched.all), `listener` removes the 8080 listener, or appends it again
(touched.listen), `minnull` removes the lowest spare row, which lies below the NULL slot and below
the port-80 listener (touched.pass2), `tuple` upserts one flow's slot with the same tuple in
SYN_RECV, or back in ESTABLISHED (touched.keys).  No other handler writes.

Expectation.  Frame i belongs to the epoch of the writers before it; Case.expect runs
oracle.rx_batch over each epoch's frames against that epoch's rows and sums the counters.

Model.  Case.sim restates rxg_rx_replay's rule (rxg::ReplayLog, csrc/rxg_replaylog.h: stale(),
absorb(), plan() with bulk_seq / scanned_seq, kHostReclassifyMax and the forced launch for F_TRUNC,
pkt_seq after fixed(); rxg_ctx::launch_writes across the bursts of a launch) over the classification
of every frame against every epoch's rows, for a default and a RXG_CFG_REPLAY_ON_DEVICE context, and
gives every launch's list, the four rxg_replay_stats figures and every writer's Touch.  Table
restates what a write adds to rxg_ctx::touched (rxg_host.cpp note_slot, rxg_tcb_upsert / _remove /
_load; TcbMirror's min_null and need_rebuild).  slices_of, blocks_of, flushes and lookaheads derive
the launch's dealing from a list as multiburst_cases does for a burst (RS = 11 slots of 1 KiB for
REC16, 4 for the all-small scratch, 6 for the class path's).

tests/test_replay_sel_cases_host.py holds every claim against the sets and the model;
tests/test_replaylog_host.py runs the model against the real ReplayLog on the CPU;
tests/test_gpu_replay_sel_edges.py runs the sets on the GPU."""
from __future__ import annotations

import functools

import numpy as np

import oracle
import pktgen
import rxg

SLICE = 64
WAVES = 4                      # rx_kernel: 256 threads
RS16 = 11                      # rxg_rx.h rx_body: RS for REC16
SLOT16 = 1024                  # ring_slot_u4(16) * 16
SMALL_SCRATCH = 4096           # small_step: ring.scratch(.., 4096, ..)
CLASS_SCRATCH = 6 * 256 + 4096  # rx_body: NF16 * 256 + 4096
K_HOST_MAX = 256               # rxg_replaylog.h kHostReclassifyMax
FILL = 0xA5
POOL_TAIL = 16384              # fill behind the last frame of every device pool
LISTENING, SYN_RECV, ESTABLISHED = 1, 3, 4
TCP_VERDICTS = (rxg.V_DISPATCH, rxg.V_RST_NOPCB, rxg.V_RST_LISTEN_NONSYN)
INF = 1 << 31

F = 257
NCLIENTS = 60
DST = pktgen.ip4(192, 168, 78, 2)
DST_RAW = pktgen.raw_of_host(DST)


def flow_tuple(f: int):
    return pktgen.ip4(10, 1, f >> 8, f & 255), 2000 + f


def client_tuple(c: int):
    return pktgen.ip4(172, 16, 0, c), 40000 + c


SPARES = [(pktgen.ip4(10, 7, 0, k), 700 + k) for k in range(2)]
L80 = (80, 0, DST_RAW, 0, LISTENING)
L8080 = (8080, 0, DST_RAW, 0, LISTENING)


def flow_row(f: int, state: int = ESTABLISHED):
    src, sport = flow_tuple(f)
    return (80, sport, DST_RAW, src, state)


ROWS = [(80, s[1], DST_RAW, s[0], ESTABLISHED) for s in SPARES] + [L80, None] + [flow_row(f) for f in range(F)] + [L8080]
SPARE_ROWS = set(ROWS[:2])


# ------------------------------------------------------------------------------------ frames ---
@functools.lru_cache(maxsize=None)
def flow_frame(f: int, ln: int) -> bytes:
    src, sport = flow_tuple(f)
    fr = pktgen.frame(src_ip=src, dst_ip=DST, sport=sport, dport=80, flags=0x10, seq=1000 + f, ack=f,
                      payload=bytes((f + t) & 0xFF for t in range(ln - 54)))
    assert len(fr) == ln
    return fr


@functools.lru_cache(maxsize=None)
def client_frame(c: int, dport: int, flags: int) -> bytes:
    src, sport = client_tuple(c)
    return pktgen.frame(src_ip=src, dst_ip=DST, sport=sport, dport=dport, flags=flags, seq=c, payload=bytes(10))


NON_TCP = {
    "arp": pktgen.frame(ethertype=0x0806, payload=bytes(10)),
    "udp": pktgen.frame(proto=17, src_ip=pktgen.ip4(10, 9, 9, 9), payload=bytes(10)),
    "l2": pktgen.frame(ethertype=0x88B5, payload=bytes(10)),
}
NON_TCP_ORDER = ("arp", "udp", "l2")


def build_frame(i: int, spec) -> bytes:
    """spec: ("flow", len) | ("cut", len): the 64-byte flow frame's first len bytes | ("syn", dport) |
    ("ack", dport) | ("arp",) | ("udp",) | ("l2",)."""
    kind = spec[0]
    if kind == "flow":
        return flow_frame(i % F, spec[1])
    if kind == "cut":
        return flow_frame(i % F, 64)[:spec[1]]
    if kind in ("syn", "ack"):
        return client_frame(i % NCLIENTS, spec[1], 0x02 if kind == "syn" else 0x10)
    return NON_TCP[kind]


def key_of_row(r):
    return ((r[0] << 16) | r[1], r[2], r[3])


def key_of_frame(f: bytes):
    """rxg_replaylog.h frame_key (frames of >= 54 bytes)."""
    return ((int.from_bytes(f[36:38], "big") << 16) | int.from_bytes(f[34:36], "big"),
            int.from_bytes(f[30:34], "little"), int.from_bytes(f[26:30], "big"))


# ------------------------------------------------------------------------- the table's writes ---
class Touch:
    """What one handler call's writes leave in rxg_ctx::touched (rxg::WriteSet)."""

    def __init__(self, keys=(), listen=(), all_=False, pass2=False):
        self.keys, self.listen, self.all, self.pass2 = list(keys), list(listen), all_, pass2

    def add(self, o):
        self.keys += o.keys
        self.listen += o.listen
        self.all |= o.all
        self.pass2 |= o.pass2

    def __bool__(self):
        return bool(self.keys or self.listen or self.all or self.pass2)


class Table:
    """tcbs[] as python rows, and what every write adds to touched.  need_rebuild: a load has not
    been pushed yet (every write then sets touched.pass2); a fix-up pushes (pushed())."""

    def __init__(self, rows):
        self.rows, self.need_rebuild = list(rows), False

    def min_null(self) -> int:
        return next((i for i, r in enumerate(self.rows) if r is None), INF)

    def _note(self, idx, t):
        if idx < len(self.rows) and self.rows[idx] is not None:
            r = self.rows[idx]
            t.keys.append(key_of_row(r))
            if r[4] == LISTENING:
                t.listen.append(r[0])

    def load(self, rows) -> Touch:
        self.rows, self.need_rebuild = list(rows), True
        return Touch(all_=True)

    def upsert(self, idx, row) -> Touch:
        t, mn = Touch(), self.min_null()
        self._note(idx, t)
        while len(self.rows) <= idx:
            self.rows.append(None)
        self.rows[idx] = row
        self._note(idx, t)
        t.pass2 = self.need_rebuild or self.min_null() != mn
        return t

    def remove(self, idx) -> Touch:
        t, mn = Touch(), self.min_null()
        self._note(idx, t)
        self.rows[idx] = None
        t.pass2 = self.need_rebuild or self.min_null() != mn
        return t

    def pushed(self):
        self.need_rebuild = False


def apply_writer(table: Table, kind, eng=None) -> Touch:
    """One writer's write on the rows and, with an engine, the same through rxg_tcb_*."""
    rows = table.rows
    if kind == "reload":
        new = rows[1:] + rows[:1]
        if eng:
            eng.tcb_load(*pktgen.table_arrays(new))
        return table.load(new)
    if kind == "listener":
        if L8080 in rows:
            idx = rows.index(L8080)
            assert idx > table.min_null()                   # the lowest NULL slot stays
            if eng:
                eng.tcb_remove(idx)
            return table.remove(idx)
        idx = len(rows)                                     # appended: no NULL slot appears
        if eng:
            eng.tcb_upsert(idx, *L8080)
        return table.upsert(idx, L8080)
    if kind == "minnull":
        idx = min(i for i, r in enumerate(rows) if r in SPARE_ROWS)
        assert idx < table.min_null() and idx < rows.index(L80)
        if eng:
            eng.tcb_remove(idx)
        return table.remove(idx)
    if kind[0] == "tuple":
        f = kind[1]
        idx = next(i for i, r in enumerate(rows) if r is not None and r[:4] == flow_row(f)[:4])
        row = flow_row(f, SYN_RECV if rows[idx][4] == ESTABLISHED else ESTABLISHED)
        if eng:
            eng.tcb_upsert(idx, row[0], row[1], row[2], row[3], row[4])
        return table.upsert(idx, row)
    raise KeyError(kind)


# -------------------------------------------------------------------------- the launch's dealing ---
def slices_of(lens) -> list:
    return [list(lens[s:s + SLICE]) for s in range(0, len(lens), SLICE)]


def blocks_of(nslices: int, max_blocks: int) -> int:
    return min((nslices + 3) // 4, max_blocks)              # rx_args: g.blocks


def is_small(sl) -> bool:
    return len(sl) == SLICE and max(sl) <= 64               # rx_body: all_small (a launch's runs are whole slices)


def need_slots(small: bool) -> int:
    return ((SMALL_SCRATCH if small else CLASS_SCRATCH) + SLOT16 - 1) // SLOT16   # RecRing::scratch: need


def flushes(sl: list, blocks: int) -> list:
    """Per wave the flushes of its ring: (slices staged, at the wave's end?)."""
    out = []
    for w in range(blocks * WAVES):
        ring, fl = [], []
        for s in range(w, len(sl), blocks * WAVES):
            if len(ring) + need_slots(is_small(sl[s])) > RS16:
                fl.append((ring, False))
                ring = []
            ring = ring + [s]
        if ring:
            fl.append((ring, True))
        out.append(fl)
    return out


def kind_of(sl: list, t: int) -> str:
    if t >= len(sl):
        return "past"
    s = sl[t]
    if is_small(s):
        return "full"
    big = [i for i, ln in enumerate(s) if ln > 64]
    if not big:
        return "partial"
    if len(s) == SLICE and big in ([0], [63]):
        return "big%d" % big[0]
    return "other"


def lookaheads(sl: list, blocks: int) -> list:
    """(wave, slice, what small_step's look-ahead finds at slice + nwaves) for every all-small slice."""
    nw = blocks * WAVES
    return [(s % nw, s, kind_of(sl, s + nw)) for s in range(len(sl)) if is_small(sl[s])]


# -------------------------------------------------------------------------------------- case ---
class Sim:
    def __init__(self):
        self.launches = []       # (burst, list of frame indices within the burst)
        self.marked = self.host = self.dev = 0
        self.seen = []           # per frame the epoch whose classification its handler saw
        self.touches = []        # (writer frame, the Touch its write left), in frame order

    @property
    def stats(self):
        return {"marked": self.marked, "host_fixups": self.host, "device_fixups": self.dev,
                "device_launches": len(self.launches)}


class Case:
    """specs: per frame its spec (build_frame).  writers: frame index -> writer kind.  bursts: the
    frame ranges of a multi-burst launch (default: one burst).  form: how the burst reaches the
    context (host | dev | strided | multi | smulti).  order: the frames' places in the pool of a dev
    form (fwd | rev | shuffle).  kind: the records handed to the replay.  max_blocks: None = the
    default and the RXG_CFG_REPLAY_ON_DEVICE context, else a capped RXG_CFG_REPLAY_ON_DEVICE one.
    checks: the ARP mirror holds half the sources, every 7th TCP frame has a payload byte flipped,
    and the replay verifies the TCP checksum."""

    def __init__(self, name, specs, writers, bursts=None, form="dev", order="fwd", kind=rxg.REC16, max_blocks=None,
                 checks=False):
        self.name, self.specs, self.writers = name, list(specs), dict(writers)
        self.n = len(self.specs)
        self.bursts = bursts or [(0, self.n)]
        self.form, self.order, self.kind, self.max_blocks, self.checks = form, order, kind, max_blocks, checks
        for i in self.writers:
            assert self.specs[i][0] == "flow", (name, i)

    @functools.cached_property
    def frames(self) -> list:
        fr = [build_frame(i, s) for i, s in enumerate(self.specs)]
        if self.checks:
            k = 0
            for i, f in enumerate(fr):
                if self.specs[i][0] not in ("flow", "syn", "ack") or i in self.writers:
                    continue
                k += 1
                if k % 7 == 0:
                    b = bytearray(f)
                    b[len(b) - 1] ^= 0x5A
                    fr[i] = bytes(b)
        return fr

    @functools.cached_property
    def lens(self) -> list:
        return [len(f) for f in self.frames]

    @functools.cached_property
    def packed(self):
        return pktgen.pack_arena(self.frames)

    @functools.cached_property
    def known_sources(self) -> list:
        """checks: the sources the ARP mirror is loaded with."""
        return sorted({int.from_bytes(f[26:30], "big") for f in self.frames})[::2]

    # --- epochs
    @functools.cached_property
    def epochs(self) -> list:
        """The rows of every epoch and the touch of the writer that closes it (as with no load pending)."""
        t, out = Table(ROWS), []
        for i in sorted(self.writers):
            rows = list(t.rows)
            t.pushed()
            out.append((rows, apply_writer(t, self.writers[i])))
        out.append((list(t.rows), None))
        return out

    def epoch_of(self, i: int) -> int:
        return sum(1 for w in self.writers if w < i)

    @functools.lru_cache(maxsize=None)
    def cls(self, e: int):
        """Every frame classified against epoch e's rows."""
        arena, off, lens = self.packed
        return oracle.rx_batch(arena, off, lens, *pktgen.table_arrays(self.epochs[e][0]))[0]["c"]

    @functools.cached_property
    def expect(self):
        """Per frame (verdict, tcb_idx, state, flags), the summed counters and the final rows."""
        arena, off, lens = self.packed
        cuts = [0] + [w + 1 for w in sorted(self.writers)] + [self.n]
        recs, cnt = [], np.zeros(rxg.NCOUNTERS, dtype=np.uint64)
        for e, (a, b) in enumerate(zip(cuts, cuts[1:])):
            if b > a:
                r, c = oracle.rx_batch(arena, off[a:b], lens[a:b], *pktgen.table_arrays(self.epochs[e][0]))
                recs.append(r["c"])
                cnt += c
        return np.concatenate(recs), cnt, self.epochs[-1][0]

    # --- the selection
    @functools.lru_cache(maxsize=None)
    def sim(self, on_device: bool) -> Sim:
        out = Sim()
        c0 = self.cls(0)
        is_tcp = np.isin(c0["verdict"], TCP_VERDICTS)
        trunc = (c0["flags"] & rxg.F_TRUNC) != 0
        keys = [key_of_frame(f) if len(f) >= 54 else None for f in self.frames]
        cur = [0] * self.n           # the epoch whose classification frame j's record holds
        table, e = Table(ROWS), 0
        launch = Touch()             # rxg_ctx::launch_writes: the writes of this launch's replays so far

        def pass2(j):
            r = self.cls(cur[j])[j]
            return r["tcb_idx"] < 0 or bool(r["flags"] & rxg.F_LISTEN)

        for b, (lo, hi) in enumerate(self.bursts):
            seq = {}
            st = dict(wseq=0, any=0, all=0, minnull=0, bulk=0, scanned=0)
            key_seq, listen_seq = {}, {}

            def absorb_lists(t):
                st["wseq"] += 1
                w = st["any"] = st["wseq"]
                if t.all:
                    st["all"] = st["bulk"] = w
                if t.pass2:
                    st["minnull"] = st["bulk"] = w
                for k in t.keys:
                    key_seq[k] = w
                for d in t.listen:
                    listen_seq[d] = w
                    st["bulk"] = w

            def stale(j):
                s = seq.get(j, 0)
                if st["any"] <= s or not is_tcp[j]:
                    return False
                if st["all"] > s or trunc[j]:
                    return True
                if key_seq.get(keys[j], 0) > s:
                    return True
                if pass2(j):
                    if st["minnull"] > s or listen_seq.get(keys[j][0] >> 16, 0) > s:
                        return True
                return False

            if b > 0 and launch:
                absorb_lists(launch)
            for i in range(lo, hi):
                if st["any"] > seq.get(i, 0) and stale(i):
                    out.marked += 1
                    batched = False
                    if on_device or trunc[i] or st["bulk"] > st["scanned"]:
                        sel = [j for j in range(i, hi) if stale(j)]
                        st["scanned"] = st["wseq"]
                        if on_device or trunc[i] or len(sel) > K_HOST_MAX:
                            out.launches.append((b, [j - lo for j in sel]))
                            for j in sel:
                                cur[j], seq[j] = e, st["wseq"]
                            out.dev += len(sel)
                            batched = True
                    if not batched:
                        cur[i], seq[i] = e, st["wseq"]
                        out.host += 1
                    table.pushed()
                out.seen.append(cur[i])
                if i in self.writers:
                    assert self.cls(cur[i])[i]["verdict"] == rxg.V_DISPATCH and not self.checks_drop(i)
                    t = apply_writer(table, self.writers[i])
                    e += 1
                    assert table.rows == self.epochs[e][0]
                    out.touches.append((i, t))
                    launch.add(t)
                    absorb_lists(t)
        return out

    def checks_drop(self, i: int) -> bool:
        """checks: the replay frees frame i for its TCP checksum."""
        r = self.cls(0)[i]
        return self.checks and r["verdict"] in TCP_VERDICTS and not (r["flags"] & rxg.F_TCP_OK)

    def sel_lens(self, launch) -> list:
        b, sel = launch
        return [self.lens[self.bursts[b][0] + j] for j in sel]


# -------------------------------------------------------------------------------------- sets ---
SIZES_M = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
CLASS_EDGES = [64, 65, 128, 129, 256, 257, 512, 513, 576, 577, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 9000]
CLASS_RANGES = [(54, 64), (65, 128), (129, 256), (257, 512), (513, 576), (577, 768), (769, 1024), (1025, 1536),
                (1537, 2048), (2049, 9000)]           # size_class 0, 1, 2, 3, 10, 8, 4, 5, 6, 7
AHEAD = ["F", "F", "F", "F", "F", "B0", "B63", "F", "F", "F", "F", "P"]   # a list slice per token, on 4 waves
AHEAD_KINDS = ["full", "partial", "big0", "big63", "past"]
WAVE_SLICES = [17, 48, 49, 97]
TRUNC_LENS = [34, 40, 53, 54]
TRUNC_N = 120
FORMS = ["host", "dev", "strided", "multi", "smulti"]
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
REWRITES_N = 1200
PASS2 = [("syn", 80), ("ack", 80), ("syn", 8080), ("ack", 8080), ("syn", 9999), ("ack", 9999)]


def tcp(m: int, ln: int = 64) -> list:
    return [("flow", ln)] * m


def mixed_specs() -> list:
    """The writer, one list slice of every edge length, then small slices past kHostReclassifyMax."""
    sl = [("flow", CLASS_EDGES[k // 3] if k % 3 == 0 and k // 3 < len(CLASS_EDGES) else 64) for k in range(64)]
    return tcp(1) + sl + tcp(256)


def holes_specs(n: int, selected) -> list:
    """Frame 0 the writer, a flow frame where selected(i), else ARP / UDP / a foreign ethertype."""
    return [("flow", 64) if i == 0 or selected(i) else (NON_TCP_ORDER[i % 3],) for i in range(n)]


def rewrites_specs(n: int, writers) -> list:
    sp = []
    for i in range(n):
        sp.append(("flow", 64) if i in writers or i % 3 != 1 else PASS2[(i // 3) % 6])
    return sp


def rewrites_writers(order: str, n: int) -> dict:
    if order == "a":
        return dict(zip([0, 100, 101, n - 2], ["reload", "minnull", "listener", ("tuple", (n - 1) % F)]))
    return dict(zip([0, 700, 701, n - 2], [("tuple", 2), "listener", "minnull", "reload"]))


HOLES = {
    "every_second": (1001, lambda i: i % 2 == 1),
    "lane63": (20000, lambda i: i % 64 == 63),
    "lane0": (20000, lambda i: i % 64 == 0),
    "last_alone": (20000, lambda i: i == 19999),
    "spread300": (20000, lambda i: i % 66 == 1 and i < 300 * 66),
}


def _build(name: str) -> Case:
    p = name.split("/")
    if p[0] == "sizes":
        return Case(name, tcp(1 + int(p[1]), int(p[2])), {0: "reload"})
    if p[0] == "holes":
        if p[1] == "reversed":
            n, sel = HOLES["every_second"]
            return Case(name, holes_specs(n, sel), {0: "reload"}, order="rev")
        n, sel = HOLES[p[1]]
        return Case(name, holes_specs(n, sel), {0: "reload"})
    if p[0] == "classes":
        if p[1] == "mixed":
            return Case(name, mixed_specs(), {0: "reload"})
        if p[1] == "per_class":  # a full list slice per size class, its two edge lengths alternating
            sp = tcp(1)
            for lo, hi in CLASS_RANGES:
                sp += [("flow", hi if (k == 5 or hi != 9000) and k % 2 else lo) for k in range(64)]
            return Case(name, sp, {0: "reload"})
        sp = tcp(1)              # ahead: all-small slices and what follows them four slices on
        for t in AHEAD:
            s = tcp(17 if t == "P" else 64)
            if t in ("B0", "B63"):
                s[int(t[1:])] = ("flow", 65)
            sp += s
        return Case(name, sp, {0: "reload"}, max_blocks=1)
    if p[0] == "waves":
        mb, s, last, body = int(p[1]), int(p[2]), p[3], p[4]
        m = 64 * s if last == "whole" else 64 * (s - 1) + 1
        sp = tcp(m)
        if body == "class":      # one 100-byte frame per list slice, on a lane of its own
            for t in range(0, m, 64):
                sp[min(t + (7 * (t // 64)) % 64, m - 1)] = ("flow", 100)
        return Case(name, tcp(1) + sp, {0: "reload"}, max_blocks=mb)
    if p[0] == "rewrites":
        w = rewrites_writers(p[1], REWRITES_N)
        return Case(name, rewrites_specs(REWRITES_N, w), w)
    if p[0] == "trunc":
        if p[1] == "no_write":
            sp = tcp(TRUNC_N + 1)
            for k, ln in enumerate(TRUNC_LENS):
                sp[1 + 30 * k] = ("cut", ln)
            return Case(name, sp, {}, form="host")
        ln, at = int(p[1]), {"first": 1, "middle": TRUNC_N // 2, "last": TRUNC_N}[p[2]]
        sp = tcp(TRUNC_N + 1)
        sp[at] = ("cut", ln)
        return Case(name, sp, {0: "reload"}, form="host")
    if p[0] == "forms":
        form, kind = p[1], int(p[2])
        w = rewrites_writers("a", REWRITES_N)
        sp = rewrites_specs(REWRITES_N, w)
        bursts = None
        if form in ("multi", "smulti"):     # bursts 1 and 2 carry no writer: re-selected whole (launch_writes.all)
            sp = sp + rewrites_specs(365, {})
            bursts = [(0, REWRITES_N), (REWRITES_N, REWRITES_N + 300), (REWRITES_N + 300, REWRITES_N + 365)]
        return Case(name, sp, w, bursts=bursts, form=form, order="shuffle" if form == "dev" else "fwd", kind=kind)
    if p[0] == "checks":
        if p[1] == "sizes257":
            return Case(name, tcp(258), {0: "reload"}, checks=True, form="host")
        if p[1] == "mixed":      # a frame read with a shorter frame's len fails its checksum
            return Case(name, mixed_specs(), {0: "reload"}, checks=True)
        n, sel = HOLES["every_second"]
        return Case(name, holes_specs(n, sel), {0: "reload"}, checks=True)
    raise KeyError(name)


NAMES = {
    "sizes": [f"sizes/{m}/{ln}" for ln in (64, 100) for m in SIZES_M],
    "holes": [f"holes/{h}" for h in HOLES] + ["holes/reversed"],
    "classes": ["classes/mixed", "classes/per_class", "classes/ahead"],
    "waves": [f"waves/{mb}/{s}/{last}/{body}" for mb in (1, 2) for s in WAVE_SLICES for last in ("whole", "one")
              for body in ("small", "class")],
    "rewrites": ["rewrites/a", "rewrites/b"],
    "trunc": [f"trunc/{ln}/{at}" for ln in TRUNC_LENS for at in ("first", "middle", "last")] + ["trunc/no_write"],
    "forms": [f"forms/{f}/{k}" for f in FORMS for k in KINDS],
    "checks": ["checks/sizes257", "checks/every_second", "checks/mixed"],
}
ALL = [n for v in NAMES.values() for n in v]


@functools.lru_cache(maxsize=None)
def get(name: str) -> Case:
    return _build(name)


def contexts(c: Case) -> list:
    """The context kinds a case runs on: (on_device, max_blocks)."""
    return [(True, c.max_blocks)] if c.max_blocks else [(False, 0), (True, 0)]
