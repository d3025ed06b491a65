"""Deterministic edge sets for the kernels of the flow trains (rxg_flow_trains_dev,
csrc/rxg_flowtrain.hip).  tests/flowtrain_cases.py holds the rule's cases; these place their
inputs from the kernels' own structure: the two left-out counters past the first wave and the
first trip of their sum (`counters`), three sort passes over several tiles with every digit live
(`passes`), a digit that lives in one wave-round of a tile (`digit`), train starts on the edges
of a ballot, a round and a tile (`starts`), a tile without a start between two that have some
(`hole`), the last lane of an emit workgroup and the widest cur_seq index (`emit`), and the
order of the tests in the record decode (`decode`).

Every set is a flowtrain_cases.Case: crafted REC48 records handed over in each kind, the frames
that carry their seq, and the claims it makes about where its edges fall.  Every expectation is
flowtrain_ref.trains.  The helpers below restate structure only (which slice a frame lies in,
which wave-round of which tile a pair lies in before each pass, which sorted position a train
starts at), never output: tests/test_flowtrain_edge_cases_host.py holds every claim against
the sets themselves and against the model."""
import numpy as np

import flowtrain_cases as cases
import rxg
from flowtrain_cases import ACK, OK, Case, cat, chain, craft, runs

fc = cases.fc
TILE = rxg.FLOW_TRAIN_TILE              # pairs per tile of the sort and of the cut
ROUND = rxg.FLOW_TRAIN_ROUND_LANES      # lanes of a sort, cut or emit workgroup: a round of a tile
SCAN = rxg.FLOW_TRAIN_SCAN_ROUND        # entries per round of a one-workgroup scan
SCAN_PER = 16                           # entries per lane of it (csrc/rxg_kernels.h kFtScanPer)
SCAN_LANES = SCAN // SCAN_PER           # its lanes: the stride of the sum over the two left-out counters
WAVE = 64                               # lanes of a wave: frames of a slice, pairs of a wave-round
SUBS = TILE // WAVE                     # wave-rounds of a tile, in list order
KINDS = [rxg.REC8, rxg.REC16, rxg.REC48]
BIG = [rxg.REC16, rxg.REC48]            # the kinds whose tcb_idx is an int32
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
NOT_OK = rxg.F_IP_OK                    # a record's flags without TCP_OK
TOP_NTCB = min(1 << 24, fc.REC8_MAX_TCB + 1)     # the largest table every record kind can name the top of


# ---------------------------------------------------------------- structure, restated ---
def kinds_of(rec48, ntcb, flags=0):
    """(segment, out of range, left out by the checksum flag) per crafted record."""
    c = rec48["c"]
    tcb, dl = c["tcb_idx"].astype(np.int64), c["datalen"].astype(np.int64)
    disp = c["verdict"] == rxg.V_DISPATCH
    inr = disp & (tcb >= 0) & (tcb < ntcb)
    ok = (c["flags"] & rxg.F_TCP_OK) != 0 if flags & rxg.FT_TCP_OK_ONLY else np.ones(len(c), bool)
    return inr & ok & (dl > 0) & (dl <= 65535), disp & ~inr, inr & ~ok


def per_slice(mask):
    """The mask's count in each slice of WAVE frames."""
    n = len(mask)
    pad = np.zeros((n + WAVE - 1) // WAVE * WAVE, np.int64)
    pad[:n] = mask
    return pad.reshape(-1, WAVE).sum(axis=1)


def pass_inputs(tcb, npasses):
    """The keys as pass p of the sort reads them, p = 0 .. npasses - 1: in packet order, then
    stably sorted on the digits below p."""
    tcb = np.asarray(tcb, np.int64)
    out = []
    for p in range(npasses):
        out.append(tcb[np.argsort(tcb & ((1 << (8 * p)) - 1), kind="stable")])
    return out


def tiles_of(keys):
    return [keys[t:t + TILE] for t in range(0, len(keys), TILE)]


def interleave(parts, seed):
    """The parts' records in one random packet order that keeps each part's own order."""
    rng = np.random.default_rng(seed)
    which = rng.permutation(np.repeat(np.arange(len(parts)), [len(p) for p in parts]))
    out = np.zeros(len(which), parts[0].dtype)
    for k, p in enumerate(parts):
        out[which == k] = p
    return out


def kinds(case):
    """The record kinds a set is handed over in."""
    return case.claims.get("kinds", KINDS)


# ------------------------------------------------- 1. the two left-out counters' sum ---
COUNTER_NTCB = 37


def counter_case(name, nslices, tail, out_at, left_at, every=False):
    """nslices full slices and `tail` more frames, all segments but: out_at / left_at are
    {slice: how many of its frames are out of range / lack TCP_OK}; with `every`, every other
    slice holds one of each as well."""
    n = nslices * WAVE + tail
    rng = np.random.default_rng(n + len(out_at) + 3 * len(left_at) + every)
    r = runs(rng.integers(0, COUNTER_NTCB, n), seed=n % 1000)
    c = r["c"]
    total = nslices + (tail > 0)
    outs, lefts = dict(out_at), dict(left_at)
    if every:
        for s in range(total):
            if s not in outs and s not in lefts:
                outs[s], lefts[s] = 1, 1
    for s in sorted(set(outs) | set(lefts)):
        size = min(WAVE, n - s * WAVE)
        no, nl = outs.get(s, 0), lefts.get(s, 0)
        assert no + nl <= size
        lanes = rng.permutation(size)[:no + nl] + s * WAVE
        c["tcb_idx"][lanes[:no]] = rng.choice([-1, COUNTER_NTCB, COUNTER_NTCB + 31], no)
        c["flags"][lanes[no:]] = NOT_OK
    r["c"] = c
    return Case(f"counters: {name}", r, COUNTER_NTCB, flags=rxg.FT_TCP_OK_ONLY,
                claims={"n": n, "slices": total, "out": sum(outs.values()), "left": sum(lefts.values()),
                        "out_at": {s: k for s, k in outs.items() if k}, "left_at": {s: k for s, k in lefts.items() if k}})


def counter_cases():
    w, l = WAVE, SCAN_LANES          # slice w: the second wave's first lane; slice l: lane 0's second trip
    return [counter_case(f"slice {w} of {w + 1} alone", w, 17, {w: 5}, {w: 3}),
            counter_case(f"slice {l} of {l + 1} alone", l, 3, {l: 2}, {l: 1}),
            counter_case("every slice, two of them whole", l, 3, {5: WAVE, l: 1}, {70: WAVE, l: 1}, every=True),
            counter_case(f"one out of range in slice {w}, none left out", w, 17, {w: 1}, {}),
            counter_case(f"one left out in slice {w}, none out of range", w, 17, {}, {w: 1})]


# the two SCAN_LANES-slice sets: 4 MB of frame slots each.  (All three layouts run; should a GPU
# parameter ever take more than a few seconds, cut these two to REC8 and REC48.)
LARGEST = SCAN_LANES * WAVE + 3


# --------------------------------------------------- 2. three passes, several tiles ---
PALETTE = [0x00, 0xFF, 0x01, 0x7F, 0x80, 0xFE, 0x10, 0x55, 0xAA, 0x33]


def pass_flows(seed=2):
    """300 flows below TOP_NTCB whose three digits each take every palette value."""
    rng = np.random.default_rng(seed)
    d = np.array(PALETTE)
    every = [(a, b, c) for a in d for b in d for c in d if (int(c) << 16 | int(b) << 8 | int(a)) < TOP_NTCB]
    pick = rng.choice(len(every), 300, replace=False)
    return np.array(sorted(int(every[k][2]) << 16 | int(every[k][1]) << 8 | int(every[k][0]) for k in pick))


def pass_cases():
    rng = np.random.default_rng(22)
    flows = pass_flows()
    n = 3 * TILE + 5
    tcb = np.concatenate([flows, rng.choice(flows, n - len(flows))])
    rng.shuffle(tcb)
    lower = 1 << 16
    return [Case("passes: three over four tiles, every digit live", runs(tcb, seed=23, p_cont=0.8), TOP_NTCB,
                 claims={"passes": 3, "tiles": 4, "S": n, "digits": 8, "multi": 50}),
            Case("passes: the same burst folded into two", runs(tcb % lower, seed=23, p_cont=0.8), lower,
                 claims={"passes": 2, "tiles": 4, "S": n, "digits": 8, "multi": 50})]


# -------------------------------------------------- 3. a digit in one wave-round only ---
def digit_positions():
    return [0, TILE - 1, 1 * WAVE + 5, 14 * WAVE + 40]


def digit_cases():
    out = []
    for tiles in (1, 2):
        for p in digit_positions():
            at = (tiles - 1) * TILE + p
            tcb = np.zeros(tiles * TILE, np.int64)
            tcb[at] = 0xFF
            out.append(Case(f"digit: 0xFF at position {p} of tile {tiles - 1} of {tiles}", runs(tcb, seed=p + tiles), 256,
                            claims={"passes": 1, "tiles": tiles, "S": tiles * TILE, "odd": (tiles - 1, p // WAVE)}))
    return out


# ----------------------------------------------------------- 4. starts on the edges ---
EDGES = [WAVE - 1, WAVE, ROUND - 1, ROUND, TILE - 1, TILE, 2 * TILE]
AFTER = [WAVE + 1, ROUND + 1, TILE + 1, 2 * TILE + 1]       # one position after each lane-0 edge
TAIL = 9                                                    # segments after the last start


def by_flows(bounds, seed):
    """All segments: the sorted list's flows change exactly at `bounds`; each flow's segments are
    contiguous, the packet order is a random merge."""
    cuts = [0] + list(bounds) + [bounds[-1] + TAIL]
    parts = [chain(k, 1000 + 100000 * k, [7] * (b - a)) for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    return interleave(parts, seed), len(parts)


def by_gaps(bounds):
    """One flow whose segments are contiguous but for a gap in sequence space before each of `bounds`."""
    n = bounds[-1] + TAIL
    seq = 1000 + 7 * np.arange(n) + 100000 * np.searchsorted(np.asarray(bounds), np.arange(n), side="right")
    return craft(np.full(n, 3), seq, 7), 5


def start_cases():
    out = []
    for b in EDGES:
        r, nt = by_flows([b], seed=b)
        out.append(Case(f"starts: a flow boundary at {b}", r, nt, claims={"firsts": [0, b], "S": b + TAIL}))
    for name, bounds in (("every edge", EDGES), ("one position after each edge", AFTER)):
        r, nt = by_flows(bounds, seed=len(bounds))
        out.append(Case(f"starts: flow boundaries at {name}", r, nt, claims={"firsts": [0] + bounds, "S": bounds[-1] + TAIL}))
        r, nt = by_gaps(bounds)
        out.append(Case(f"starts: gaps in one flow at {name}", r, nt, claims={"firsts": [0] + bounds, "S": bounds[-1] + TAIL}))
    return out


# -------------------------------------------------------------- 5. a tile without a start ---
def hole_case():
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 1461, 2 * TILE + 7)
    r = interleave([craft(np.zeros(5), 50000 * np.arange(5) + 9, 11), chain(1, 4242, lens),
                    craft(np.full(3, 2), 70000 * np.arange(3) + 1, 13)], seed=5)
    return Case("hole: a train over a whole tile between two tiles with starts", r, 3, cur_seq={1: 4242},
                claims={"T": 9, "S": 2 * TILE + 15, "tiles": 3, "hole": 1, "long": (5, 2 * TILE + 7, int(lens.sum())),
                        "cap_trains": [9, 8, 5]})


# ---------------------------------------------------------------------- 6. emit edges ---
def head_case(ntcb):
    """Flow ntcb - 1's one train is a HEAD by cur_seq[ntcb - 1] alone: the entries its index cut to
    16 and to 8 bits names hold other flows' seqs."""
    top = ntcb - 1
    lo16, lo8 = top & 0xFFFF, top & 0xFF
    others = sorted({lo16, lo8, 1} - {top})
    parts = [chain(top, 0x51525354, [100, 100, 100])] + [chain(f, 0x01020304 + 0x100 * k, [50, 50]) for k, f in enumerate(others)]
    seq_of = {f: 0x01020304 + 0x100 * k for k, f in enumerate(others)}
    cur = {top: 0x51525354}
    for f in sorted({lo16, lo8} - {top}):
        cur[f] = seq_of[1]                       # another flow's seq: neither flow f's nor the top flow's
    return Case(f"emit: HEAD on flow ntcb - 1 of {ntcb}", interleave(parts, seed=ntcb % 97), ntcb, cur_seq=cur,
                claims={"heads": 1, "head_flow": top, "T": len(parts), "passes": cases.passes_needed(ntcb)})


def emit_cases():
    out = []
    for T in (ROUND - 1, ROUND, ROUND + 1):
        tcb = np.random.default_rng(T).permutation(T)
        out.append(Case(f"emit: {T} trains of one segment", runs(tcb, seed=T), T + 3, claims={"T": T, "S": T}))
    parts = [chain(k, 900 + 5000 * k, [20, 30]) for k in range(ROUND)]
    out.append(Case(f"emit: {ROUND} trains of two segments", interleave(parts, seed=6), ROUND,
                    claims={"T": ROUND, "S": 2 * ROUND}))
    return out + [head_case(ntcb) for ntcb in (257, 65537, TOP_NTCB)]


# --------------------------------------------------------------------- 7. decode order ---
def decode_cases():
    """One frame each beside two segments of flow ntcb - 1 of 3."""
    ntcb = 3
    seg = chain(2, 500, [10, 10])
    order = cat(seg,
                craft([3], 1, 10, flags=NOT_OK),                            # out of range and not TCP_OK: out
                craft([3], 2, 0),                                           # out of range, datalen 0: out
                craft([2], 3, 0, flags=NOT_OK),                             # not TCP_OK, datalen 0: left
                craft([3], 4, 10, flags=NOT_OK, verdict=rxg.V_ARP),         # not DISPATCH: nothing
                craft([-1], 5, 0, flags=NOT_OK))                            # all three at once: out
    out = [Case("decode: range before the checksum flag before datalen", order, ntcb, flags=rxg.FT_TCP_OK_ONLY,
                claims={"counts": [2, 1, 3, 1]})]
    for name, idx, ks in (("INT32_MIN and INT32_MAX", [INT32_MIN, INT32_MAX], BIG),
                          ("-1 and the 8-byte record's largest", [-1, fc.REC8_MAX_TCB], KINDS)):
        r = cat(seg, craft(idx, 6, 10), craft(idx, 7, 0, flags=NOT_OK), craft(idx, 8, 10, verdict=rxg.V_DROP_L2))
        out.append(Case(f"decode: tcb_idx {name}", r, ntcb, flags=rxg.FT_TCP_OK_ONLY,
                        claims={"counts": [2, 1, 4, 0], "kinds": ks}))
    return out


def edge_cases():
    """Every set, in the order of the families above."""
    return (counter_cases() + pass_cases() + digit_cases() + start_cases() + [hole_case()] + emit_cases() +
            decode_cases())
