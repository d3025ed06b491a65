"""Deterministic edge sets for the multi-burst launch (rxg_rx_bursts_dev, rxg_rx_bursts_strided_dev:
the MULTI instantiations of rx_kernel, csrc/rxg_rx.h and rxg_rx_core.h), a model of how a launch
deals its slices, and the expectations.

Layout of every case.  Frames are pktgen.frame with valid checksums against TABLE: frame i of burst
j carries the tuple of table row j * 64 + i % 64, and its payload length is (i // 64) % 11, so a
record's tcb_idx names burst and lane and its datalen the slice within the burst: a record written
for the wrong burst, lane or slice shows in REC8.  All bursts' off64 lie end to end in one buffer
and all len in a second, each closed by TAIL entries that name slot 0 with length 64; slot 0 of the
pool holds a valid frame of a tuple (table row SPARE_ROW) no burst uses.  The records lie in one
buffer pre-filled with FILL, burst j's followed by GUARD records before the next burst's; the REC8
buffer starts 8 bytes in, so a burst's records are 8 but not 16 bytes aligned.  The expectation is
that whole buffer built from oracle.rx_batch over the bursts' concatenation.  The strided form puts
frame i of burst j at slot 1 + j + i * k (k bursts, stride64 = k; twice that where a set holds
frames over 64 bytes), unused slots and slot tails FILL.

tests/test_multiburst_cases_host.py holds every claim made here against the sets and the model;
tests/test_gpu_multiburst_edges.py runs them."""
from __future__ import annotations

import functools

import numpy as np

import oracle
import pktgen
import rxg

SLICE = 64
GUARD = 8                # records between two bursts' outputs
FILL = 0xA5
TAIL = 192               # descriptor entries behind the last burst's
BIG = 65                 # the smallest frame that leaves the all-small path
PARTIAL = 17             # frames of a partial slice where a set does not say otherwise
SIZES = [1, 63, 64, 65, 129]

# ------------------------------------------------------------------ constants of the sources ---
K_MAX_BURSTS = 32                            # rxg_kernels.h kMaxBursts
K_DEEP_SLICES_PER_WAVE = 16                  # rxg_rx_core.h kDeepSlicesPerWave
WAVES = 4                                    # rx_kernel: 256 threads, nwaves = 4 * gridDim.x
RS = {8: 22, 16: 11, 48: 4}                  # rxg_rx.h rx_body: RS (no MSG)
SLOT_BYTES = {8: 512, 16: 1024, 48: 3072}    # rxg_rx.h ring_slot_u4(MODE) * 16
NF = {8: 6, 16: 6, 48: 10}                   # rxg_rx_frames.h NF16 (REC8 and REC16) / NF48
NEVER_DEEP = (48,)                           # rxg_kernels.hip launch_rx: case 48 has no DEEP kernel
SMALL_SCRATCH = 4096                         # small_step / small_step2: ring.scratch(.., 4096, ..)


def class_scratch(kind: int) -> int:
    return NF[kind] * 256 + 4096             # rx_body: ring.scratch(.., NF * 256 + 4096, ..)


# ----------------------------------------------------------------------------- table, frames ---
NB_TABLE = 128
DST = pktgen.ip4(192, 168, 78, 2)
SPARE_ROW = NB_TABLE * SLICE
SPARE_TUPLE = (pktgen.ip4(10, 9, 9, 9), 999)


def src_of(j: int, lane: int) -> int:
    return pktgen.ip4(10, 1, j, lane)


ROWS = [(80, 1024 + r % SLICE, pktgen.raw_of_host(DST), src_of(r // SLICE, r % SLICE), pktgen.ESTABLISHED)
        for r in range(NB_TABLE * SLICE)]
ROWS.append((80, SPARE_TUPLE[1], pktgen.raw_of_host(DST), SPARE_TUPLE[0], pktgen.ESTABLISHED))
TCB, LIVE = pktgen.table_arrays(ROWS)


@functools.lru_cache(maxsize=None)
def frame_of(j: int, lane: int, ln: int) -> bytes:
    f = pktgen.frame(src_ip=src_of(j, lane), dst_ip=DST, sport=1024 + lane, dport=80, seq=1000 * j + lane,
                     payload=bytes((j + lane + t) & 0xFF for t in range(ln - 54)))
    assert len(f) == ln
    return f


SPARE = pktgen.frame(src_ip=SPARE_TUPLE[0], dst_ip=DST, sport=SPARE_TUPLE[1], dport=80, payload=bytes(10))
assert len(SPARE) == 64


def small(n: int) -> list:
    """Lengths of a burst of n small frames: the payload length names the slice."""
    return [54 + (i // SLICE) % 11 for i in range(n)]


def put(lens: list, at: dict) -> list:
    lens = list(lens)
    for i, ln in at.items():
        lens[i] = ln
    return lens


# ------------------------------------------------------------------------------------- model ---
class Launch:
    """One kernel launch as rx_args (rxg_rx.h) numbers it: empty bursts dropped first."""

    def __init__(self, caller, ns):
        self.caller, self.n = list(caller), list(ns)     # caller's burst index / frames, per kernel burst
        self.slice0, s = [], 0
        for n in self.n:
            self.slice0.append(s)
            s += (n + 63) // 64
        self.nslices = s
        self.multi = len(self.n) > 1                     # launch_mode: a.nbursts > 1

    def blocks(self, max_blocks: int) -> int:
        return min((self.nslices + 3) // 4, max_blocks)  # rx_args: g.blocks

    def deep(self, max_blocks: int, kind: int) -> bool:
        return kind not in NEVER_DEEP and self.nslices >= K_DEEP_SLICES_PER_WAVE * self.blocks(max_blocks) * WAVES


def plan(ns) -> list:
    """launch_bursts (rxg_host.cpp): chunks of kMaxBursts; launch_rx makes no launch of no slices."""
    out = []
    for j0 in range(0, len(ns), K_MAX_BURSTS):
        kept = [(j, n) for j, n in enumerate(ns[j0:j0 + K_MAX_BURSTS], j0) if n]
        if kept:
            out.append(Launch([j for j, _ in kept], [n for _, n in kept]))
    return out


class Slice:
    def __init__(self, k, j, t, lens):
        self.k, self.j, self.t = k, j, t                 # kernel burst, caller's burst, slice within the burst
        self.n_burst = len(lens)
        part = lens[t * SLICE:(t + 1) * SLICE]
        self.frames = len(part)
        self.big = tuple(i for i, ln in enumerate(part) if ln > 64)
        self.small = self.frames == SLICE and not self.big      # rx_body: all_small
        self.last_partial = self.frames < SLICE


def slices_of(launch: Launch, lens_of) -> list:
    """The launch's slices in launch order; lens_of(j): the caller's burst j's frame lengths."""
    return [Slice(k, j, t, lens_of(j)) for k, (j, n) in enumerate(zip(launch.caller, launch.n))
            for t in range((n + 63) // 64)]


def wave_slices(nslices: int, blocks: int, wave: int):
    return range(wave, nslices, blocks * WAVES)          # rx_body: s = wave, wave + nwaves, ...


def need_slots(kind: int, is_small: bool) -> int:
    b = SMALL_SCRATCH if is_small else class_scratch(kind)
    return (b + SLOT_BYTES[kind] - 1) // SLOT_BYTES[kind]   # RecRing::scratch: need


def flushes(sl: list, kind: int, blocks: int) -> list:
    """Per wave the flushes of its RecRing: (slot contents as Slice objects, at the wave's end?).
    scratch() flushes when the free slots are fewer than the slice's scratch needs; put() takes one."""
    out = []
    for w in range(blocks * WAVES):
        ring, fl = [], []
        for s in wave_slices(len(sl), blocks, w):
            if len(ring) + need_slots(kind, sl[s].small) > RS[kind]:
                fl.append((ring, False))
                ring = []
            ring = ring + [sl[s]]
        if ring:
            fl.append((ring, True))
        out.append(fl)
    return out


def kind_of(sl: list, t: int) -> str:
    """What a run's look-ahead finds at launch slice t."""
    if t >= len(sl):
        return "past"
    s = sl[t]
    if s.small:
        return "full"
    if not s.big and s.frames < SLICE:
        return "one" if s.n_burst == 1 else "partial"
    if s.frames == SLICE and s.big in ((0,), (63,)):
        return "big%d" % s.big[0]
    return "other"


def run_events(sl: list, blocks: int, deep: bool) -> list:
    """(wave, where, what, burst edge?, slice the step processes) for every look-ahead of every
    all-small run.  Plain kernel (small_step): where = 'd1', the test of slice s + nwaves.  DEEP
    (small_step2): 'entry' is pend's first value (slice s + nwaves, rx_body), 'd2' the test of slice
    s + 2 nwaves with pend set, 'd2clear' the same slice when pend is clear (nxt2 must be false)."""
    nw, n, ev = blocks * WAVES, len(sl), []

    def edge(a, b):
        return b < n and sl[a].k != sl[b].k

    for w in range(nw):
        s = w
        while s < n:
            if not sl[s].small:
                s += nw
                continue
            if not deep:
                while True:
                    c = kind_of(sl, s + nw)
                    ev.append((w, "d1", c, edge(s, s + nw), s))
                    s += nw
                    if c != "full":
                        break
                continue
            c = kind_of(sl, s + nw)
            ev.append((w, "entry", c, edge(s, s + nw), s))
            pend = c == "full"
            while True:
                c2 = kind_of(sl, s + 2 * nw)
                ev.append((w, "d2" if pend else "d2clear", c2, s + nw < n and edge(s + nw, s + 2 * nw), s))
                cont, pend = pend, pend and c2 == "full"
                s += nw
                if not cont:
                    break
    return ev


# -------------------------------------------------------------------------------------- case ---
class Case:
    """bursts: per burst the list of its frame lengths.  null_empties: empty bursts carry NULL
    pointers.  mem_order: the order in which the bursts' ranges lie in the three buffers.  split:
    every second burst's records lie in a second buffer."""

    def __init__(self, name, bursts, null_empties=False, mem_order=None, split=False):
        self.name, self.lens, self.null_empties, self.split = name, [list(b) for b in bursts], null_empties, split
        self.k = len(self.lens)
        self.ns = [len(b) for b in self.lens]
        self.mem_order = list(range(self.k)) if mem_order is None else list(mem_order)
        assert sorted(self.mem_order) == list(range(self.k))
        self.wide = any(ln > 64 for b in self.lens for ln in b)
        self.launches = plan(self.ns)

    def lens_of(self, j):
        return self.lens[j]

    def frames(self, j) -> list:
        return [frame_of(j, i % SLICE, ln) for i, ln in enumerate(self.lens[j])]

    # --- the pool, list form: slot 0, then the bursts' frames in order
    @functools.cached_property
    def packed(self):
        offs, pos, parts = [], 1, [SPARE]
        for j in range(self.k):
            o = []
            for f in self.frames(j):
                o.append(pos)
                pos += (len(f) + 63) // 64
                parts.append(f)
            offs.append(np.array(o, dtype=np.uint32))
        pool = np.full(pos * 64, FILL, dtype=np.uint8)
        at = [0] + [int(x) for o in offs for x in o]
        for a, f in zip(at, parts):
            pool[a * 64:a * 64 + len(f)] = np.frombuffer(f, dtype=np.uint8)
        return pool, offs

    # --- the pool, strided form
    @property
    def stride64(self) -> int:
        return (2 if self.wide else 1) * self.k

    def slot0(self, j) -> int:
        return 1 + (2 if self.wide else 1) * j

    @functools.cached_property
    def strided(self):
        per = 2 if self.wide else 1
        top = 1
        for j in range(self.k):
            for i, ln in enumerate(self.lens[j]):
                top = max(top, self.slot0(j) + i * self.stride64 + max(per, (ln + 63) // 64))
        pool = np.full(top * 64, FILL, dtype=np.uint8)
        used = np.zeros(top, dtype=bool)
        used[0] = True
        pool[:64] = np.frombuffer(SPARE, dtype=np.uint8)
        for j in range(self.k):
            for i, f in enumerate(self.frames(j)):
                a, nsl = self.slot0(j) + i * self.stride64, (len(f) + 63) // 64
                assert not used[a:a + nsl].any(), (self.name, j, i, "frames overlap in the strided pool")
                used[a:a + nsl] = True
                pool[a * 64:a * 64 + len(f)] = np.frombuffer(f, dtype=np.uint8)
        return pool

    # --- descriptors: all off64 end to end, all len end to end, TAIL entries behind each
    @functools.cached_property
    def desc(self):
        _, offs = self.packed
        start, pos = [0] * self.k, 0
        for j in self.mem_order:
            start[j] = pos
            pos += self.ns[j]
        off_all = np.zeros(pos + TAIL, dtype=np.uint32)
        len_all = np.full(pos + TAIL, 64, dtype=np.uint16)
        for j in range(self.k):
            off_all[start[j]:start[j] + self.ns[j]] = offs[j]
            len_all[start[j]:start[j] + self.ns[j]] = self.lens[j]
        return off_all, len_all, start

    # --- records
    def rec_layout(self, kind: int):
        """(buffer, byte offset) of every burst's records and the buffers' sizes."""
        lead = 8 if kind == rxg.REC8 else 0
        size, where = [lead, lead] if self.split else [lead], [None] * self.k
        for j in self.mem_order:
            b = j % 2 if self.split else 0
            where[j] = (b, size[b])
            size[b] += (self.ns[j] + GUARD) * kind
        return where, size

    @functools.cached_property
    def oracle(self):
        pool, offs = self.packed
        live = [j for j in range(self.k) if self.ns[j]]
        if not live:
            return np.zeros(0, dtype=rxg.REC48_DTYPE), np.zeros(rxg.NCOUNTERS, dtype=np.uint64)
        off = np.concatenate([offs[j] for j in live])
        lens = np.concatenate([np.array(self.lens[j], dtype=np.uint16) for j in live])
        return oracle.rx_batch(pool, off, lens, TCB, LIVE)

    def expect(self, kind: int):
        """The record buffers as a correct call leaves them, and the counters."""
        exp, cnt = self.oracle
        recs = {rxg.REC8: lambda: rxg.rec8_pack(exp["c"]), rxg.REC16: lambda: exp["c"], rxg.REC48: lambda: exp}[kind]()
        raw = np.ascontiguousarray(recs).view(np.uint8).reshape(len(exp), kind)
        where, size = self.rec_layout(kind)
        imgs = [np.full(s, FILL, dtype=np.uint8) for s in size]
        pos = 0
        for j in range(self.k):
            b, o = where[j]
            imgs[b][o:o + self.ns[j] * kind] = raw[pos:pos + self.ns[j]].reshape(-1)
            pos += self.ns[j]
        return imgs, cnt

    def describe(self, kind: int, b: int, byte: int) -> str:
        where, _ = self.rec_layout(kind)
        for j in range(self.k):
            bb, o = where[j]
            if bb == b and o <= byte < o + (self.ns[j] + GUARD) * kind:
                i = (byte - o) // kind
                return (f"burst {j} (n {self.ns[j]}) " +
                        (f"frame {i} (slice {i // SLICE}, lane {i % SLICE}, len {self.lens[j][i]})" if i < self.ns[j]
                         else f"guard record {i - self.ns[j]}"))
        return "the buffer's lead"


# -------------------------------------------------------------------------------------- sets ---
def closed_walk(m: int) -> list:
    """A closed walk over every ordered pair of m nodes, loops included (m * m + 1 nodes)."""
    unused = {a: list(range(m)) for a in range(m)}
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if unused[v]:
            stack.append(unused[v].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


PAIR_WALK = [SIZES[i] for i in closed_walk(len(SIZES))]


def pairs_bursts(big_last: bool) -> list:
    return [put(small(n), {n - 1: BIG}) if big_last else small(n) for n in PAIR_WALK]


# empties: k = 6, the bursts that carry frames
EMPTY_K = 6
EMPTY_FULL = [65, 129, 64, 1, 63, 130]
EMPTY_PATTERNS = {
    "first": [0], "last": [5], "two_mid": [2, 3],
    "only_0": [1, 2, 3, 4, 5], "only_3": [0, 1, 2, 4, 5], "only_5": [0, 1, 2, 3, 4],
    "all": [0, 1, 2, 3, 4, 5],
}

COUNT_KS = [1, 2, 31, 32, 33, 63, 64, 65, 97]
COUNT_NS = [1, 65]
COUNT_HOLES = {"k64_first_chunk_empty": (64, range(0, 32)), "k64_second_chunk_empty": (64, range(32, 64)),
               "k40_empty_across_the_cut": (40, range(30, 34))}


def ring_class_bursts() -> list:
    """32 x 129 with one 100-byte frame in every slice (on a lane of its own per slice), and the
    one 1 500-byte frame as the last frame of the last burst."""
    out = []
    for j in range(32):
        out.append(put(small(129), {7 * j % 64: 100, 64 + (7 * j + 3) % 64: 100, 128: 100}))
    out[31][128] = 1500
    return out


# runs: a slice per token, a burst per list
F, P, O, B0, B63 = "F", "P", "O", "B0", "B63"
RUNS_SHORT = [[F, F, F], [F, F, P], [B0], [O], [F, F, F], [F, B63], [F, F, F], [F, F]]
RUNS_DEEP = [[F, F, F, F]] * 12 + [[P], [B0, B63], [O], [F, F, F], [F, B0, P], [O], [B63, F, F], [F, F], [F, F, F]]
RUN_KINDS = ["full", "partial", "big0", "big63", "one", "past"]


def tokens_burst(tokens: list) -> list:
    assert all(t not in (P, O) for t in tokens[:-1]) and (O not in tokens or tokens == [O])
    n = sum({P: PARTIAL, O: 1}.get(t, SLICE) for t in tokens)
    at = {}
    for s, t in enumerate(tokens):
        if t == B0:
            at[s * SLICE] = BIG
        if t == B63:
            at[s * SLICE + 63] = BIG
    return put(small(n), at)


def _build(name: str) -> Case:
    parts = name.split("/")
    if parts[0] == "pairs":
        return Case(name, pairs_bursts(parts[1] == "big_last"))
    if parts[0] == "empties":
        hole = EMPTY_PATTERNS[parts[1]]
        return Case(name, [[] if j in hole else small(EMPTY_FULL[j]) for j in range(EMPTY_K)],
                    null_empties=parts[2] == "null")
    if parts[0] == "counts":
        if parts[1] in COUNT_HOLES:
            k, hole = COUNT_HOLES[parts[1]]
            return Case(name, [[] if j in hole else small(65) for j in range(k)], null_empties=True)
        return Case(name, [small(int(parts[2]))] * int(parts[1]))
    if parts[0] == "ring":
        return Case(name, {"small129": lambda: [small(129)] * 32, "class129": ring_class_bursts,
                           "x32_65": lambda: [small(65)] * 32, "x31_65": lambda: [small(65)] * 31}[parts[1]]())
    if parts[0] == "runs":
        return Case(name, [tokens_burst(t) for t in {"short": RUNS_SHORT, "deep": RUNS_DEEP}[parts[1]]])
    if parts[0] == "order":
        k = len(PAIR_WALK)
        return Case(name, pairs_bursts(False), mem_order=range(k - 1, -1, -1), split=parts[1] == "split")
    raise KeyError(name)


NAMES = {
    "pairs": ["pairs/small", "pairs/big_last"],
    "empties": [f"empties/{p}/{v}" for p in EMPTY_PATTERNS for v in ("valid", "null")],
    "counts": [f"counts/{k}/{n}" for n in COUNT_NS for k in COUNT_KS] + [f"counts/{h}" for h in COUNT_HOLES],
    "ring": ["ring/small129", "ring/class129", "ring/x32_65", "ring/x31_65"],
    "runs": ["runs/short", "runs/deep"],
    "order": ["order/reversed", "order/split"],
}
ALL = [n for v in NAMES.values() for n in v]
WITH_REC48 = ("pairs", "ring", "counts")


@functools.lru_cache(maxsize=None)
def get(name: str) -> Case:
    return _build(name)
