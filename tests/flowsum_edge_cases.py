"""Deterministic edge sets for the kernels of the per-flow summary (rxg_flow_sums_dev,
csrc/rxg_flowsum.hip).  tests/flowsum_cases.py holds the rule's cases; these aim at the kernels' own
machinery: the seven places where two frames of one flow are combined (`meet`), the workgroup-end
LDS merge (`lds`), a wave's slice run and its cuts (`runs`), the two left-out counters (`left`), the
record decode (`decode`), the frame read of seq and ack (`frames`), the output limit (`cap`) and
the tile scan (`scan`).

The call is a pure function of records and frames (include/rxg.h), so every set is crafted REC48
records handed over in each kind (flowsum_cases.as_kind) and frames that carry their seq and ack.
Every expectation is flowsum_ref.summaries.  `Structure` restates how launch_flow_sum and
flow_sum_acc place the work for a context with max_blocks 1, 2 or 3 (below any CU count, so the
grid is known without a GPU); it predicts structure only, never output: a set uses it to show that
it reaches the place it claims to reach (tests/test_flowsum_edge_cases_host.py holds every claim
made below against the sets themselves)."""
from __future__ import annotations

import numpy as np

import flowsum_cases as cases
import rxg

SLICE = 64
GUARD = 8
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
BIG = [rxg.REC16, rxg.REC48]                  # the kinds whose tcb_idx and datalen are int32
BLOCKS = [1, 2, 3]
TILE = rxg.FLOW_SUM_TILE_TCBS
ROUND = rxg.FLOW_SUM_SCAN_TILES
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
REC8_MAX_DATALEN = (1 << 17) - 1 - 128        # rxg.h: bits 14-30 of w1 hold datalen + 128
REC8_MIN_DATALEN = -120                       # rxg.h: total_length - 60 - 60
ARP = rxg.V_ARP
NONE, MIXED = -1, -2                          # Structure.uniform: no counted frame / more than one flow


# ----------------------------------------------------------------- the structural model ---
def grid(n: int, max_blocks: int):
    """(nslices, ablocks, per, [(s0, s1) per wave]) of flow_sum_acc for n frames."""
    nslices = (n + SLICE - 1) // SLICE
    ablocks = min((nslices + 3) // 4, max_blocks)
    nwaves = 4 * ablocks
    per = (nslices + nwaves - 1) // nwaves
    runs = []
    for w in range(nwaves):
        s0 = min(w * per, nslices)
        runs.append((s0, min(s0 + per, nslices)))
    return nslices, ablocks, per, runs


def counted_mask(c, ntcb: int, flags: int = 0):
    """(counted, out of range, left out by the checksum flag) per record of REC16_DTYPE `c`."""
    tcb = c["tcb_idx"].astype(np.int64)
    disp = c["verdict"] == rxg.V_DISPATCH
    inr = disp & (tcb >= 0) & (tcb < ntcb)
    ok = (c["flags"] & rxg.F_TCP_OK) != 0 if flags & rxg.FS_TCP_OK_ONLY else np.ones(len(c), bool)
    return inr & ok, disp & ~inr, inr & ~ok


class Structure:
    """Where flow_sum_acc takes the frames of one burst on a context with `max_blocks`.

    uniform[s]   the slice's one flow; NONE without a counted frame; MIXED with more than one
    carried[w]   [(flow, [slices])]: the flows wave w carries in registers, in order
    commits[w]   the flows wave w adds to memory because the flow changed
    mixed[w]     [(slice, the flow carried at that time or NONE, the slice's flows)]
    ends[w]      the flow wave w hands to the LDS merge (NONE: nothing carried)
    groups[g]    the four endings of workgroup g"""

    def __init__(self, c, ntcb, flags, max_blocks):
        self.tcb = c["tcb_idx"].astype(np.int64)
        self.datalen = c["datalen"].astype(np.int64)
        self.counted, self.out, self.nok = counted_mask(c, ntcb, flags)
        self.n = len(c)
        self.nslices, self.ablocks, self.per, self.runs = grid(self.n, max_blocks)
        self.uniform = []
        for s in range(self.nslices):
            t = np.unique(self.tcb[s * SLICE:(s + 1) * SLICE][self.counted[s * SLICE:(s + 1) * SLICE]])
            self.uniform.append(NONE if len(t) == 0 else int(t[0]) if len(t) == 1 else MIXED)
        self.carried, self.commits, self.mixed, self.ends = [], [], [], []
        for s0, s1 in self.runs:
            flow, car, com, mix = NONE, [], [], []
            for s in range(s0, s1):
                u = self.uniform[s]
                if u == NONE:
                    continue
                if u == MIXED:
                    mix.append((s, flow, set(self.flows_of(s))))
                    continue
                if u != flow:
                    if flow != NONE:
                        com.append(flow)
                    flow = u
                    car.append((u, [s]))
                else:
                    car[-1][1].append(s)
            self.carried.append(car)
            self.commits.append(com)
            self.mixed.append(mix)
            self.ends.append(flow)
        self.groups = [self.ends[4 * g:4 * g + 4] for g in range(self.ablocks)]

    def flows_of(self, s):
        sl = slice(s * SLICE, (s + 1) * SLICE)
        return self.tcb[sl][self.counted[sl]].tolist()

    def wave_of(self, s):
        return next(w for w, (s0, s1) in enumerate(self.runs) if s0 <= s < s1)

    def empty_waves(self):
        return [w for w, (s0, s1) in enumerate(self.runs) if s0 == s1]

    def lane_bytes(self, slices):
        """data_bytes per lane over `slices` of one carried flow: what the lane's registers hold."""
        out = np.zeros(SLICE, np.int64)
        for s in slices:
            sl = slice(s * SLICE, min((s + 1) * SLICE, self.n))
            d = np.where(self.counted[sl] & (self.datalen[sl] > 0), self.datalen[sl], 0)
            out[:len(d)] += d
        return out

    def left_of_wave(self, w):
        s0, s1 = self.runs[w]
        sl = slice(s0 * SLICE, s1 * SLICE)
        return int(self.out[sl].sum()), int(self.nok[sl].sum())


# --------------------------------------------------------------------------- the cases ---
def frames_of(rec48, lens=54, fill=0xEE):
    """flowsum_cases.frames_for for frames of any length: seq and ack at bytes 38..46, `fill`
    everywhere else, cut (or filled up) to lens[i] bytes."""
    n = len(rec48)
    lens = np.broadcast_to(np.asarray(lens), (n,)).tolist()
    head = np.full((n, 64), fill, np.uint8)
    head[:, 38:42] = rec48["seq"].astype(">u4").view(np.uint8).reshape(n, 4)
    head[:, 42:46] = rec48["ack"].astype(">u4").view(np.uint8).reshape(n, 4)
    return [head[i, :ln].tobytes() if ln <= 64 else head[i].tobytes() + bytes([fill]) * (ln - 64)
            for i, ln in enumerate(lens)]


class Case:
    """One burst: REC48 records, the kinds it is handed over in, the max_blocks values its claims
    are made for, and `claim(structure)`, which asserts them."""

    def __init__(self, name, rec48, ntcb, kinds=KINDS, blocks=BLOCKS, flags=0, claim=None, lens=54, fill=0xEE):
        self.name, self.rec48, self.ntcb, self.kinds, self.blocks, self.flags = name, rec48, ntcb, list(kinds), list(blocks), flags
        self.claim, self.lens, self.fill, self.n = claim or (lambda st: None), lens, fill, len(rec48)

    def recs(self, kind):
        return cases.as_kind(self.rec48, kind)

    def frames(self, kind):
        """The frames for that kind (None for REC48, which needs none), built once."""
        if kind == rxg.REC48:
            return None
        if not hasattr(self, "_frames"):
            self._frames = frames_of(self.rec48, self.lens, self.fill)
        return self._frames

    def structure(self, max_blocks):
        return Structure(self.rec48["c"], self.ntcb, self.flags, max_blocks)

    def __repr__(self):
        return self.name


def with_fields(r, **kw):
    c = r["c"]
    for k, v in kw.items():
        if k in ("seq", "ack"):
            r[k] = np.asarray(v).astype(np.uint32)
        else:
            c[k] = v
    r["c"] = c
    return r


def filler(tcb, seed, flags=cases.OK):
    """Counted frames of the flows `tcb` with random fields."""
    rng = np.random.default_rng(seed)
    n = len(tcb)
    return cases.craft(tcb, seq=rng.integers(0, 2**32, n), ack=rng.integers(0, 2**32, n), datalen=rng.integers(-3, 1461, n),
                       tcp_flags=rng.choice([0x10, 0x18, 0x11], n), flags=flags, state=rng.integers(0, 7, n))


# ------------------------------------------------------------------------------- meet ---
F = 777                       # the planted flow
MEET_NTCB = 4096
PLACES = ["a wave reduction", "b register carry", "c lds merge", "d two workgroups", "e per-lane atomics",
          "f atomics under a carry", "g committed and met again"]
MEET_PER = 3                  # every wave takes slices 3 w .. 3 w + 2


def fr(seq, ack, dl, fl, st):
    return dict(seq=seq, ack=ack, datalen=dl, tcp_flags=fl, state=st)


def variants(kind):
    """name -> the planted flow's frames in burst order; the first frame's state differs from every
    later one's.  `bytes` (int32 datalen only) passes 2^32 with its third frame; `flags` carries one
    distinct bit per frame and the half that adds 0x80 arrives last."""
    big = kind != rxg.REC8
    v = {"hi": [fr(0x7FFFFFFF, 0x80000000, 1, 0x10, 3), fr(0x80000000, 0x7FFFFFFF, 0, 0x10, 4)],
         "hi swapped": [fr(0x80000000, 0x7FFFFFFF, 0, 0x10, 2), fr(0x7FFFFFFF, 0x80000000, 1, 0x10, 4)],
         "top": [fr(0xFFFFFFFE, 0xFFFFFFFF, -1, 0x7F, 1), fr(0xFFFFFFFF, 0xFFFFFFFE, INT32_MIN if big else REC8_MIN_DATALEN, 0xFF, 4)],
         "zero": [fr(0, 0, 0, 0, 6), fr(0, 0, 1, 0, 4)],
         "flags": [fr(100 + k, 200 - k, 0, 1 << k, 0 if k == 0 else 4) for k in range(8)]}
    if big:
        v["bytes"] = [fr(5, 6, INT32_MAX, 0x10, 5), fr(7, 8, INT32_MAX, 0x10, 4), fr(9, 10, INT32_MAX, 0x18, 4)]
    return v


def split(place, vname, frames):
    """The planted frames as the sides of the place.  Two sides; the register carry takes `bytes`
    one frame per slice in one lane, so that the lane's own sum passes 2^32."""
    if place[0] == "b" and vname == "bytes":
        return [[f] for f in frames]
    h = len(frames) // 2 if vname != "bytes" else 2
    return [frames[:h], frames[h:]]


def meet_positions(place, nsides):
    """[(slice, first lane)] per side, and how the other lanes of those slices are filled:
    'idle' (non-DISPATCH records that name the planted flow) or 'mix' (counted frames of distinct
    filler flows)."""
    p = place[0]
    if p == "a":
        return [(4, 5), (4, 40)], {4: "idle"}
    if p == "b":
        return [(3, 17), (4, 17), (5, 17)][:max(nsides, 2)], {3: "idle", 4: "idle", 5: "idle"}
    if p == "c":
        return [(5, 9), (8, 50)], {5: "idle", 8: "idle"}
    if p == "d":
        return [(4, 9), (16, 50)], {4: "idle", 16: "idle"}
    if p == "e":
        return [(4, 3), (4, 58)], {4: "mix"}
    if p == "f":
        return [(3, 7), (4, 20)], {3: "idle", 4: "mix"}
    return [(3, 30), (5, 31)], {3: "idle", 5: "idle"}


def meet_case(place, vname, kind, mb):
    sides = split(place, vname, variants(kind)[vname])
    pos, fill = meet_positions(place, len(sides))
    nslices = 4 * mb * MEET_PER
    n = nslices * SLICE
    r = filler(100 + np.arange(n) // SLICE, seed=7 * mb + len(vname))      # slice s: one uniform filler flow 100 + s
    where = []
    for s, how in fill.items():
        sl = slice(s * SLICE, (s + 1) * SLICE)
        if how == "idle":                        # ignored records that name the planted flow and carry every bit
            r[sl] = cases.craft(np.full(SLICE, F), seq=0xFFFFFFFF, ack=0xFFFFFFFF, datalen=1460, tcp_flags=0xFF, verdict=ARP, state=5)
        else:                                    # 64 distinct counted flows
            r[sl] = filler(2000 + np.arange(SLICE), seed=s)
    for (s, lane), side in zip(pos, sides):
        for k, f in enumerate(side):
            i = s * SLICE + lane + k
            r[i:i + 1] = cases.craft([F], seq=f["seq"], ack=f["ack"], datalen=f["datalen"], tcp_flags=f["tcp_flags"], state=f["state"])
            where.append(i)
    p = place[0]

    def claim(st):
        assert st.per == MEET_PER and st.ablocks == mb and len(st.runs) == 4 * mb
        idx = np.nonzero(st.counted & (st.tcb == F))[0].tolist()
        assert idx == where, "only the planted frames are counted for the planted flow"
        sl = [i // SLICE for i in where]
        w = [st.wave_of(s) for s in sl]
        if p == "a":
            assert len(set(sl)) == 1 and st.uniform[sl[0]] == F and len(where) >= 2
        elif p == "b":
            assert len(set(w)) == 1 and (F, sorted(set(sl))) in st.carried[w[0]] and len(set(sl)) >= 2
            assert len({i % SLICE for i in where}) == len(sides[0]), "the same lanes in every slice"
            if vname == "bytes":
                assert st.lane_bytes(sorted(set(sl)))[where[0] % SLICE] > 2**32, "the lane's own sum passes 2^32"
        elif p == "c":
            assert w[0] != w[-1] and w[0] // 4 == w[-1] // 4 and st.ends[w[0]] == st.ends[w[-1]] == F
            assert st.groups[w[0] // 4].count(F) == 2
        elif p == "d":
            assert w[0] // 4 != w[-1] // 4
            assert all(F in [f for f, _ in st.carried[x]] for x in (w[0], w[-1]))
        elif p == "e":
            assert len(set(sl)) == 1 and st.uniform[sl[0]] == MIXED and st.flows_of(sl[0]).count(F) == len(where)
        elif p == "f":
            assert len(set(w)) == 1 and st.uniform[sl[0]] == F and st.uniform[sl[-1]] == MIXED
            assert (sl[-1], F, set(st.flows_of(sl[-1]))) in st.mixed[w[0]], "the atomics land while F is carried"
        else:
            assert len(set(w)) == 1 and F in st.commits[w[0]] and st.ends[w[0]] == F
            assert [f for f, _ in st.carried[w[0]]].count(F) == 2
        if vname == "bytes":
            assert int(st.datalen[where].sum()) > 2**32 > int(st.datalen[where[:-1]].sum())

    return Case(f"meet {place}, {vname}, max_blocks {mb}", r, MEET_NTCB, kinds=[kind], blocks=[mb], claim=claim)


def meet_cases(place, mb):
    if place[0] == "d" and mb == 1:
        return []
    return [meet_case(place, v, kind, mb) for kind in KINDS for v in variants(kind)]


# -------------------------------------------------------------------------------- lds ---
LDS_PATTERNS = ["AAAA", "AABB", "ABAB", "ABBA", "ABCA", "A.A.", "...A", "ABCD"]
LDS_FLOW = {"A": 31, "B": 32, "C": 2047, "D": 2048}


def lds_case(pattern, kind):
    """Four slices on max_blocks 1: wave k's one slice holds 64 frames of the pattern's k-th flow
    ('.': no counted frame).  int32 datalen kinds carry 2^31 - 1 in every lane: a wave's sum is
    about 2^37 and the LDS merge adds numbers that are already past 2^32."""
    rng = np.random.default_rng(sum(map(ord, pattern)))
    n = 4 * SLICE
    tcb = np.repeat([LDS_FLOW.get(ch, 5) for ch in pattern], SLICE)
    r = filler(tcb, seed=int(rng.integers(1 << 30)))
    if kind != rxg.REC8:
        with_fields(r, datalen=np.where(rng.random(n) < 0.7, INT32_MAX, rng.integers(-5, 5, n)))
    idle = np.repeat([ch == "." for ch in pattern], SLICE)
    with_fields(r, verdict=np.where(idle, rxg.V_RST_NOPCB, rxg.V_DISPATCH))

    def claim(st):
        assert st.ablocks == 1 and st.per == 1
        assert st.groups == [[LDS_FLOW.get(ch, NONE) for ch in pattern]]
        assert all(not c for c in st.commits) and all(not m for m in st.mixed)

    return Case(f"lds {pattern}", r, 2 * TILE, kinds=[kind], blocks=[1], claim=claim)


# ------------------------------------------------------------------------------- runs ---
RUN_PATTERNS = {"one flow": lambda s: 5 + 0 * s, "a flow per slice": lambda s: 10 + s, "a flow per two slices": lambda s: 10 + s // 2}


def run_nslices(mb):
    nw = 4 * mb
    return [nw - 1, nw, nw + 1, 2 * nw - 1, 2 * nw, 2 * nw + 1, 3 * nw + 1]


def run_case(pattern, mb, nslices, last_full, kind):
    n = SLICE * nslices - (0 if last_full else SLICE - 1)
    tcb = RUN_PATTERNS[pattern](np.arange(n) // SLICE)
    r = filler(tcb, seed=nslices * 3 + mb)

    def claim(st):
        nw = 4 * min(mb, (nslices + 3) // 4)
        per = -(-nslices // nw)
        assert st.per == per and len(st.runs) == nw and st.nslices == nslices
        assert st.empty_waves() == [w for w in range(nw) if w * per >= nslices]
        assert all(st.ends[w] == NONE for w in st.empty_waves())
        for w, (s0, s1) in enumerate(st.runs):
            flows = [int(tcb[s * SLICE]) for s in range(s0, s1)]
            distinct = [f for k, f in enumerate(flows) if k == 0 or f != flows[k - 1]]
            assert [f for f, _ in st.carried[w]] == distinct and st.commits[w] == distinct[:-1]
            assert st.ends[w] == (distinct[-1] if distinct else NONE)
        # where `per` cuts a flow's train: the waves that carry a part of the same flow
        if pattern == "one flow":
            assert sum(len(c) for c in st.carried) == nw - len(st.empty_waves())
        if not last_full:
            assert n % SLICE == 1

    return Case(f"runs {pattern}, max_blocks {mb}, {nslices} slices, n {n}", r, 64, kinds=[kind], blocks=[mb], claim=claim)


def run_cases(mb):
    out = []
    for pattern in RUN_PATTERNS:
        for k, ns in enumerate(run_nslices(mb)):
            for full in (False, True):
                out.append(run_case(pattern, mb, ns, full, KINDS[(k + full + len(pattern)) % 3]))
    return out


# ------------------------------------------------------------------------------- left ---
def bad_tcbs(ntcb):
    return [-1, INT32_MIN, ntcb, ntcb + 31, 1 << 24, INT32_MAX]


NOT_TCP_OK = 0xFF & ~rxg.F_TCP_OK       # every other bit of the record's flags (REC8 keeps six of them)


def left_cases():
    """Bursts of 16 slices: with max_blocks 2 each of the eight waves of two workgroups takes two."""
    out = []
    n, ntcb = 16 * SLICE, 500
    lane = np.arange(n) % SLICE
    sl = np.arange(n) // SLICE
    bad = np.array(bad_tcbs(ntcb))

    def claims(whole=(), waves=(), uniform=None, out_n=None, nok_n=None, counted_n=None):
        """whole: slices without a counted frame; waves: the counters every wave of two workgroups
        adds to; uniform: what every slice is; the totals."""
        def claim(st):
            assert all(st.uniform[s] == NONE for s in whole)
            if st.ablocks == 2 and st.nslices == 16:
                assert st.per == 2
                for w in range(8):
                    o, k = st.left_of_wave(w)
                    assert ("out" not in waves or o > 0) and ("nok" not in waves or k > 0), w
            assert uniform is None or all(u == uniform for u in st.uniform)
            assert out_n is None or int(st.out.sum()) == out_n
            assert nok_n is None or int(st.nok.sum()) == nok_n
            assert counted_n is None or int(st.counted.sum()) == counted_n
        return claim

    # 1. whole slices of DISPATCH records out of range (every int32 edge), no counted frame anywhere
    r = filler(bad[(lane + sl) % len(bad)], seed=1)
    out.append(Case("left whole slices out of range, nothing counted", r, ntcb, kinds=BIG,
                    claim=claims(whole=range(16), waves=["out"], out_n=n, nok_n=0, counted_n=0)))
    # 2. the same for every kind (-1 is REC8's only index outside a table) and a counted slice at the end
    r = filler(np.where(sl < 15, -1, 7), seed=2, flags=0x3F)
    out.append(Case("left whole slices of -1", r, ntcb, claim=claims(whole=range(15), out_n=15 * SLICE, counted_n=SLICE)))
    # 3. whole slices lacking TCP_OK with every other flags bit set, under RXG_FS_TCP_OK_ONLY
    whole = [s for s in range(16) if s % 4 != 3]
    for kinds, bits in ((BIG, 0xFF), ([rxg.REC8], 0x3F)):
        r = filler(3 + (sl % 5), seed=3, flags=np.where(sl % 4 == 3, bits, bits & NOT_TCP_OK))
        out.append(Case(f"left whole slices without TCP_OK, flags of {bits:#x}", r, ntcb, kinds=kinds, flags=rxg.FS_TCP_OK_ONLY,
                        claim=claims(whole=whole, waves=["nok"], out_n=0, nok_n=12 * SLICE)))
    # 4. both kinds mixed with counted frames in every slice
    rng = np.random.default_rng(4)
    what = rng.integers(0, 3, n)
    r = filler(np.where(what == 1, bad[rng.integers(0, len(bad), n)], rng.integers(0, 40, n)), seed=4,
               flags=np.where(what == 2, NOT_TCP_OK, 0xFF))
    out.append(Case("left both kinds mixed with counted frames", r, ntcb, kinds=BIG, flags=rxg.FS_TCP_OK_ONLY,
                    claim=claims(waves=["out", "nok"], uniform=MIXED, out_n=int((what == 1).sum()), nok_n=int((what == 2).sum()))))
    assert (what == 1).sum() > 300 and (what == 2).sum() > 300
    # 5. one flow fills every slice but a few left-out lanes: the uniform path with both counters
    what = np.where(lane % 7 == 3, 1, np.where(lane % 5 == 1, 2, 0))
    r = filler(np.where(what == 1, -1, 9), seed=5, flags=np.where(what == 2, NOT_TCP_OK & 0x3F, 0x3F))
    out.append(Case("left lanes inside uniform slices", r, ntcb, flags=rxg.FS_TCP_OK_ONLY,
                    claim=claims(waves=["out", "nok"], uniform=9, out_n=int((what == 1).sum()), nok_n=int((what == 2).sum()))))
    # 6. every other verdict naming an in-range flow: ignored, not counted as left out
    for kinds, nv in ((BIG, 255), ([rxg.REC8], 7)):
        r = with_fields(filler(np.where(sl < 12, 11, 12), seed=6, flags=np.where(sl < 14, 0, 0x3F)), verdict=np.where(sl < 12, 1 + (np.arange(n) % nv), 0))
        out.append(Case(f"left the {nv} other verdicts are ignored", r, ntcb, kinds=kinds, flags=rxg.FS_TCP_OK_ONLY,
                        claim=claims(whole=range(14), out_n=0, nok_n=2 * SLICE, counted_n=2 * SLICE)))
    # 7. REC8's largest index on the largest table, beside -1
    r = filler(np.where(lane % 2 == 0, cases.REC8_MAX_TCB, -1)[:130], seed=7, flags=0x3F)
    out.append(Case("left REC8's largest index", r, rxg.FS_MAX_NTCB, claim=claims(out_n=65, counted_n=65)))
    return out


# ----------------------------------------------------------------------------- decode ---
def decode_case(kind):
    """A flow per value: every tcp_flags bit and 0xFF, every state the kind can carry, datalen at
    the kind's extremes; then flows of two frames whose first frame differs from the second."""
    big = kind != rxg.REC8
    flags = [1 << k for k in range(8)] + [0xFF, 0]
    states = list(range(7)) + [rxg.STATE_NONE] + ([8, 10, 0xFE] if big else [])
    dls = [INT32_MIN, -1, 0, 1, INT32_MAX, 65481] if big else [REC8_MIN_DATALEN, -1, 0, 1, REC8_MAX_DATALEN, 65481]
    rows = [(fl, 4, 0) for fl in flags] + [(0x10, st, 0) for st in states] + [(0x10, 4, d) for d in dls]
    two = [(0, a, b) for a in states for b in (4, rxg.STATE_NONE) if a != b]
    tcb = list(range(len(rows))) + [len(rows) + k // 2 for k in range(2 * len(two))]
    r = filler(np.array(tcb), seed=kind)
    with_fields(r, tcp_flags=[x[0] for x in rows] + [0x10] * (2 * len(two)),
                state=[x[1] for x in rows] + [s for _, a, b in two for s in (a, b)],
                datalen=[x[2] for x in rows] + [1] * (2 * len(two)))
    perm = np.random.default_rng(kind).permutation(len(rows))      # the single frames shuffled; the pairs keep their order
    r[:len(rows)] = r[:len(rows)][perm]
    return Case(f"decode records of {kind}", r, len(rows) + len(two), kinds=[kind])


# ----------------------------------------------------------------------------- frames ---
FRAME_LENS = [0] + list(range(37, 48)) + [64, 65, 0x7FFF, 0x8000, 0xFFFF]


def frames_case(lens=FRAME_LENS, seed=0):
    """A flow per frame length (and one more frame of 54 bytes per flow with small seq / ack, so a
    frame that reads as zero is seen): seq and ack have no zero byte, everything else in the
    frame is 0xFF, and the pool holds 0xFF beyond every frame."""
    lens = list(lens)
    k = len(lens)
    r = cases.craft(np.arange(2 * k) % k, seq=0xA1B2C3D4, ack=0xE5F60718)
    r[k:] = cases.craft(np.arange(k), seq=0x00000102, ack=0x00000001)
    return Case(f"frames of {len(lens)} lengths", r, k, kinds=[rxg.REC8, rxg.REC16], lens=lens + [54] * k, fill=0xFF)


def pool_list(frames, order, beyond=0xFF):
    """(pool, off64, len): frame order[k] is the k-th in the pool, every frame on its own 64-byte
    slots (an empty one too), `beyond` wherever no frame byte lies."""
    slots = [max(1, (len(f) + 63) // 64) for f in frames]
    off = np.zeros(len(frames), np.uint32)
    at = 1
    for i in order:
        off[i] = at
        at += slots[i]
    pool = np.full((at + 1) * 64, beyond, np.uint8)
    for f, o in zip(frames, off.tolist()):
        pool[o * 64:o * 64 + len(f)] = np.frombuffer(f, np.uint8)
    return pool, off, np.array([len(f) for f in frames], np.uint16)


def pool_strided(frames, slot0, stride64, beyond=0xFF):
    """(pool, off64, len, (slot0, stride64)): frame i at slot slot0 + i * stride64."""
    assert all(len(f) <= 64 * stride64 for f in frames)
    off = (slot0 + np.arange(len(frames)) * stride64).astype(np.uint32)
    pool = np.full((slot0 + len(frames) * stride64 + 1) * 64, beyond, np.uint8)
    for f, o in zip(frames, off.tolist()):
        pool[o * 64:o * 64 + len(f)] = np.frombuffer(f, np.uint8)
    return pool, off, np.array([len(f) for f in frames], np.uint16), (slot0, stride64)


def frame_forms():
    """[(name, case, build)]: build(frames) gives pool, off64, len and, for a strided pool, its
    geometry."""
    every = frames_case()
    order = np.random.default_rng(5).permutation(every.n).tolist()
    small = frames_case([ln for ln in FRAME_LENS if ln <= 64])
    mid = frames_case([ln for ln in FRAME_LENS if ln <= 128])
    assert order != sorted(order)
    return [("list ascending", every, lambda f: pool_list(f, range(len(f))) + (None,)),
            ("list shuffled", every, lambda f: pool_list(f, order) + (None,)),
            ("list descending", every, lambda f: pool_list(f, range(len(f) - 1, -1, -1)) + (None,)),
            ("stride 1 from slot 3", small, lambda f: pool_strided(f, 3, 1)),
            ("stride 2 from slot 1", mid, lambda f: pool_strided(f, 1, 2)),
            ("stride 1024 from slot 7", every, lambda f: pool_strided(f, 7, 1024))]


# -------------------------------------------------------------------------------- cap ---
def cap_case(kind):
    """150 flows: ranks 31 / 32 sit at a bitmap word's edge, ranks 63 / 64 at a tile's."""
    rng = np.random.default_rng(9)
    flows = np.concatenate([np.arange(40), np.arange(TILE - 24, TILE + 40), 2 * TILE + rng.choice(3 * TILE, 46, replace=False)])
    flows = np.sort(flows)
    assert len(flows) == 150 and flows[31] == 31 and flows[32] == 32 and flows[63] == TILE - 1 and flows[64] == TILE
    tcb = np.concatenate([flows, rng.choice(flows, 250)])
    rng.shuffle(tcb)
    return Case(f"cap records of {kind}", filler(tcb, seed=10), 5 * TILE, kinds=[kind])


def caps(m):
    return [0, 1, 31, 32, 33, 63, 64, 65, m - 1, m, m + 1, 2**32 - 1, 2**32, 2**32 + 1, 2**64 - 1]


# ------------------------------------------------------------------------------- scan ---
SCAN_NTCB = [(ROUND - 1) * TILE, ROUND * TILE - 1, ROUND * TILE, ROUND * TILE + 1, rxg.FS_MAX_NTCB]


def scan_flows(ntcb):
    ntiles = (ntcb + TILE - 1) // TILE
    t = np.arange(ntiles)
    parts = [t[t % 5 > j] * TILE + (t[t % 5 > j] * 37 + j * 509) % TILE for j in range(4)]      # t % 5 flows in tile t
    for edge in range(ROUND, ntiles + 1, ROUND):                                                # beside each round edge
        for tile in (edge - 1, edge):
            parts.append(np.array([tile * TILE, tile * TILE + TILE - 1]))
    for tile in (ROUND - 1, ROUND):                                                             # two full tiles
        parts.append(tile * TILE + np.arange(TILE))
    flows = np.unique(np.concatenate(parts))
    return flows[flows < ntcb]


def scan_case(ntcb):
    flows = scan_flows(ntcb)
    rng = np.random.default_rng(ntcb % 1000)
    tcb = np.concatenate([flows, rng.choice(flows, 1500)])
    rng.shuffle(tcb)
    assert len(tcb) < 30000
    c = Case(f"scan ntcb {ntcb}", filler(tcb, seed=11), ntcb, kinds=[rxg.REC16])
    c.flows = flows
    return c
