"""Deterministic edge sets for the kernel of the received-option parse (rxg_rx_opts_dev,
csrc/rxg_rxopt.hip: rx_opts_parse).  tests/rxopt_cases.py holds the rule's cases; these aim at
the kernel's own machinery: the length masks of frame bytes 52..95 at every length, the chunk-5
test (O > 26 and len > 80) on every lane, the candidate test on records the test writes, the walk
loop at every round count, the three bad-length tests at every (O, p, l), the aligned-timestamp
compare and its neighbours, and the grid stride past a wave's first slice.

The call is a pure function of frames and records (include/rxg.h), so nothing here is a real
burst.  A frame is cut from a byte template (no valid checksums: the parse reads frame byte 46 and
bytes 54..93 only); its verdict comes from a record the test writes in the documented layouts with
every other bit random (txreset_cases.make_recs).  What follows a frame's last byte in a pool is
rxopt_cases.POISON in the frame's own phase, as in rxopt_cases.poisoned_arena.  Every expectation
is rxopt_ref.parse, cached by what the rule reads: (len, frame[46], frame[54:94]).
tests/test_rxopt_edge_cases_host.py holds every claim made below against the sets themselves."""
from __future__ import annotations

import functools

import numpy as np

import rxg
import rxopt_cases as cases
import rxopt_ref as ref
import txreset_cases as tc

SLICE = 64
GUARD = 8
LANES = cases.GENERAL_LANES                  # 0, 1, 31, 32, 33, 62, 63
EDGE_LANES = [0, 31, 32, 63]
CAND = np.array(ref.CANDIDATE_VERDICTS, dtype=np.uint8)
OTHER = np.array([v for v in range(6) if v not in ref.CANDIDATE_VERDICTS], dtype=np.uint8)
NOP, EOL = cases.NOP, cases.EOL
mss, wscale, sack_perm, sack, timestamp, aligned_ts = (cases.mss, cases.wscale, cases.sack_perm, cases.sack,
                                                       cases.timestamp, cases.aligned_ts)

# ---------------------------------------------------------------------------- frames ---
HDR = bytes((37 * j + 11) & 0xFF for j in range(54))      # bytes 0..53 of every frame but byte 46
_POISON = np.frombuffer(cases.POISON, np.uint8)


def poison(nbytes: int, start: int = 0) -> np.ndarray:
    """What bytes start .. start + nbytes of a frame's slot hold where the frame does not: POISON
    by the offset from frame byte 54.  Slots begin on 64-byte lines, so the phase is a pool's."""
    return _POISON[(np.arange(start, start + nbytes) - 54) % 16]


_TAIL = poison(65536).tobytes()


def frame(d: int, opts: bytes = b"", ln: int | None = None) -> bytes:
    """`ln` bytes (default: up to the end of `opts`) of a frame with data_off nibble d and `opts`
    from byte 54 on.  Behind them the frame goes on with the poison, so a walk that leaves O meets
    options.  The low nibble of byte 46 is not zero: the kernel is to shift it out."""
    f = HDR[:46] + bytes([(d << 4) | ((7 * d + 3) & 0xF)]) + HDR[47:] + opts
    if ln is None:
        return f
    return f[:ln] if ln <= len(f) else f + _TAIL[len(f):ln]


def seg(opts: bytes, ln: int | None = None) -> bytes:
    """A frame whose data_off says exactly `opts` (a multiple of 4, at most 40 bytes)."""
    assert len(opts) % 4 == 0 and len(opts) <= 40
    return frame(5 + len(opts) // 4, opts, ln)


def opt_len(f: bytes) -> int:
    d = f[46] >> 4 if len(f) > 46 else 0
    return 0 if d < 5 else 4 * d - 20


def is_far(f: bytes) -> bool:
    """The kernel loads chunk 5 (frame bytes 80..95) for this frame."""
    return opt_len(f) > 26 and len(f) > 80


# ----------------------------------------------------------------------------- model ---
@functools.lru_cache(maxsize=None)
def _parse(ln: int, b46: bytes, body: bytes) -> tuple:
    return ref.as_tuple(ref.parse((bytes(46) + b46 + bytes(7) + body)[:ln]))


def model(f: bytes) -> tuple:
    """rxopt_ref.parse(f) as a tuple in rxopt_ref.FIELDS order.  A frame of 94 bytes or more has
    every byte the rule reads, so its length stands for all of them."""
    return _parse(min(len(f), 94), f[46:47], f[54:94])


def want(frames, verdicts) -> np.ndarray:
    """rxopt_ref.records(frames, verdicts) through the cache."""
    out = np.zeros(len(frames), dtype=rxg.RX_OPT_DTYPE)
    for i in np.nonzero(np.isin(verdicts, CAND))[0].tolist():
        out[i] = model(frames[i])
    return out


def walk(f: bytes):
    """The rule's walk over f, counted the way the kernel runs it: (rounds, events, read).
    rounds: options looked at, the end-of-list or bad one included; 0 for a frame that never walks
    (O == 0, or the aligned-timestamp shortcut).  events: (p, kind, l, no_length, short, over) per
    option that is no end of list and no no-operation, l None without a length byte.  read: the
    option byte positions whose value decides the record (kinds, lengths, the values of MSS, window
    scale and timestamp; SACK blocks stay in the frame)."""
    n, size = len(f), opt_len(f)

    def b(j):
        return f[54 + j] if 54 + j < n else 0

    if size == 0:
        return 0, [], set()
    if size == 12 and bytes(b(j) for j in range(4)) == cases.ALIGNED_TS:
        return 0, [], set(range(12))
    p, rounds, events, read = 0, 0, [], set()
    while p < size:
        rounds += 1
        k = b(p)
        read.add(p)
        if k == 0:
            break
        if k == 1:
            p += 1
            continue
        if p + 1 >= size:
            events.append((p, k, None, True, False, False))
            break
        ln = b(p + 1)
        read.add(p + 1)
        short, over = ln < 2, ln >= 2 and p + ln > size
        events.append((p, k, ln, False, short, over))
        if short or over:
            break
        if (k, ln) in ((2, 4), (3, 3), (8, 10)):
            read |= set(range(p + 2, p + ln))
        p += ln
    return rounds, events, read


# ------------------------------------------------------------------------------ pools ---
def _scatter(arena, starts, frames, lens):
    joined = np.frombuffer(b"".join(frames), np.uint8)
    first = np.cumsum(lens) - lens
    arena[np.repeat(starts - first, lens) + np.arange(joined.size)] = joined


class Case:
    """One call's inputs: frames, the verdict each one's record carries (default: the three
    candidate verdicts in turn) and, per frame, what the set says about it (meta)."""

    def __init__(self, name, frames, verdicts=None, meta=None):
        self.name, self.frames, self.n = name, list(frames), len(frames)
        self.verdicts = (CAND[np.arange(self.n) % 3] if verdicts is None else np.asarray(verdicts, np.uint8)).copy()
        self.meta = meta
        self.lens = np.array([len(f) for f in self.frames], dtype=np.int64)
        assert self.verdicts.size == self.n and (meta is None or len(meta) == self.n)

    def recs(self, rec_kind: int, seed: int = 0) -> np.ndarray:
        return tc.make_recs(self.verdicts, rec_kind, 7919 * seed + rec_kind + self.n)

    @functools.cached_property
    def want(self) -> np.ndarray:
        return want(self.frames, self.verdicts)

    def packed(self):
        """(pool, off64, len): the frames one after another on 64-byte lines; from a frame's end to
        its last line's end the poison.  The pool ends with the last frame's last line."""
        slots = (self.lens + 63) // 64
        off = np.cumsum(slots) - slots
        arena = poison(max(int(slots.sum()), 1) * 64).copy()
        _scatter(arena, off * 64, self.frames, self.lens)
        return arena, off.astype(np.uint32), self.lens.astype(np.uint16)

    def strided(self, slot0: int = 3):
        """(pool, off64, len, (slot0, stride64)): frame i at slot0 + i * stride64, the poison
        wherever no frame byte lies."""
        stride64 = max(1, (int(self.lens.max()) + 63) // 64)
        off = slot0 + np.arange(self.n, dtype=np.int64) * stride64
        arena = poison((slot0 + self.n * stride64) * 64).copy()
        arena[:slot0 * 64] = 0x08
        _scatter(arena, off * 64, self.frames, self.lens)
        return arena, off.astype(np.uint32), self.lens.astype(np.uint16), (slot0, stride64)


# --------------------------------------------------------------------------- len_grid ---
# (A) the aligned timestamp first, then options to the end, the last two with values the record shows
BODY_A = (aligned_ts(0xA1A2A3A4, 0xB1B2B3B4) + mss(0x05B4) + sack_perm() + wscale(9) + NOP + sack(1, 0x0C0D0E00)
          + wscale(12) + NOP + mss(0x7172))
# (B) unaligned and dense; the last option is a timestamp at p = 30, so tsecr is option bytes 36..39
BODY_B = wscale(5) + mss(1337) + sack(2, 0x7000) + sack_perm() + bytes([30, 3, 0x4B]) + timestamp(0xC1C2C3C4, 0xD1D2D3D4)
BODY_C = b"\xff" * 40
# (D) what A and B leave open: at len 67, 73, 77, 78 and 82..85 both have a length byte or a value the
# record does not show at the cut, so one byte read past len would not tell.  Here those are kinds and
# a timestamp's value (the poison's two no-operations fall on option bytes 30 and 31)
BODY_D = NOP * 24 + timestamp(0xE1E2E3E4, 0xF1F2F3F4) + NOP * 2 + mss(0x7374)
BODIES = {"A": BODY_A, "B": BODY_B, "C": BODY_C, "D": BODY_D}
assert all(len(b) == 40 for b in BODIES.values()) and BODY_B[30:32] == bytes([8, 10])
GRID_LENS = list(range(131))
LONG_LENS = [1514, 65535]
LANE_BLOCK = SLICE * (len(LANES) + 1)      # the frames in front of len_grid's grid


def _far(k):       # O > 26 and len > 80
    return frame(12 + k % 4, BODY_B if k % 2 else BODY_A, 81 + (5 * k) % 50)


def _near(k):      # O > 26, len <= 80
    return frame(12 + k % 4, BODY_A if k % 2 else BODY_B, 54 + (7 * k) % 27)


def _short(k):     # nothing of the options
    return frame(15, BODY_B, (5 * k) % 54)


def _low(k):       # len > 80, O <= 24
    return frame(5 + k % 7, BODY_A, 81 + k % 40)


def len_grid() -> Case:
    """Seven slices in which lane 0, 1, 31, 32, 33, 62 or 63 alone holds a frame that loads
    chunk 5 (meta "far"), among frames with O > 26 / len <= 80, short ones and long ones with
    O <= 24 (meta "near", "short", "low"); one slice where every lane holds one; then every len
    0..130 at every data_off nibble for the four bodies (meta (len, d, body name)), in an order
    that mixes lengths and nibbles inside every slice.  All candidates."""
    frames, meta = [], []
    others = (_near, _short, _low, _near)
    for lane in LANES:
        for k in range(SLICE):
            make = _far if k == lane else others[k % 4]
            frames.append(make(k + lane))
            meta.append({_far: "far", _near: "near", _short: "short", _low: "low"}[make])
    frames += [_far(k) for k in range(SLICE)]
    meta += ["far"] * SLICE
    grid = [(ln, d, name) for ln in GRID_LENS for d in range(16) for name in BODIES]
    assert np.gcd(2501, len(grid)) == 1
    for i in range(len(grid)):
        ln, d, name = grid[(2501 * i) % len(grid)]
        frames.append(frame(d, BODIES[name], ln))
        meta.append((ln, d, name))
    return Case("len_grid", frames, meta=meta)


def len_grid_long() -> Case:
    """len 1 514 and 65 535 at every nibble for the four bodies, every other frame; between them
    frames of 0..130 bytes.  (A set of its own: at a fixed stride every slot is 1 024 lines.)"""
    frames, meta = [], []
    for i, (ln, d, name) in enumerate((ln, d, name) for ln in LONG_LENS for d in range(16) for name in BODIES):
        short = (37 * i) % 131, (5 * i) % 16, "ABCD"[(i + 1) % 4]
        for m in ((ln, d, name), short):
            frames.append(frame(m[1], BODIES[m[2]], m[0]))
            meta.append(m)
    return Case("len_grid_long", frames, meta=meta)


# --------------------------------------------------------------------------- verdicts ---
SHORT_CANDIDATES = {0: 0, 1: 1, 31: 46, 32: 47, 33: 53, 63: 54}    # lane -> len


def verdict_frames():
    """64 frames, one per lane: truncated ones of 0, 1, 46, 47, 53 and 54 bytes (data_off 15, so
    all but the last are BAD_DOFF or CUT with nothing walked), walkers, aligned timestamps,
    option-less ones."""
    out = []
    for k in range(SLICE):
        if k in SHORT_CANDIDATES:
            out.append(frame(15, BODY_A, SHORT_CANDIDATES[k]))
        elif k % 4 == 0:
            out.append(seg(aligned_ts(0x51000000 + k, 0x52000000 + k), 66 + k))
        elif k % 4 == 1:
            out.append(frame(15, BODY_B[:30] + timestamp(0x53000000 + k, 0x54000000 + k), 94 + k))
        elif k % 4 == 2:
            out.append(seg(b"", 54 + k))
        else:
            out.append(seg(NOP * (k % 9) + mss(0x5500 + k) + NOP * (8 - k % 9)))
    return out


def verdicts() -> Case:
    """Six slices of the same 64 frames; lane k of slice s carries verdict (k + s) mod 6, so every
    frame meets every verdict on its lane."""
    fr = verdict_frames()
    v = [(k + s) % 6 for s in range(6) for k in range(SLICE)]
    return Case("verdicts", fr * 6, verdicts=v, meta=[(k, (k + s) % 6) for s in range(6) for k in range(SLICE)])


# ----------------------------------------------------------------------------- rounds ---
MAX_ROUNDS = 40


def rounds_frame(r: int, u: int) -> bytes:
    """A frame whose walk takes exactly r rounds and whose last option carries u where an option
    fits there: no-operations, then a timestamp (r <= 31) or an MSS (r <= 37) and the end of list,
    with an MSS behind it that is never to be read; r = 38 ends in a window scale, 39 in
    SACK-permitted, and 40 is 40 no-operations."""
    if r == 1:
        return seg(mss(0x4000 + u))
    if r <= 31:
        last = timestamp(0x61000000 + u, 0x62000000 + u)
    elif r <= 37:
        last = mss(0x4000 + u)
    elif r == 38:
        return seg(NOP * 37 + wscale(0x80 + u))
    elif r == 39:
        return seg(NOP * 38 + sack_perm())
    else:
        return seg(NOP * 40)
    body = NOP * (r - 2) + last + EOL
    behind = 40 - len(body)
    return seg(body + (mss(0xDEAD) + NOP * (behind - 4) if behind >= 4 else NOP * behind))


def base_rounds():
    """Per lane of the base slice: lanes 0..39 take 1 + 7k mod 40 rounds (every count once, 40 on
    lane 17), lanes 40..63 take 1 + 3k mod 39 (1..39)."""
    return [1 + (7 * k) % 40 if k < 40 else 1 + (3 * k) % 39 for k in range(SLICE)]


def never_walks(k: int) -> bytes:
    return seg(aligned_ts(0x63000000 + k, 0x64000000 + k), 66 + k % 30) if k % 2 else seg(b"", 54 + k % 30)


def rounds() -> Case:
    """Slice 0: the base slice.  Slices 1..4: the same with the 40-round frame swapped to lane 0,
    31, 32, 63.  Slices 5..16: a 40-round frame on lane 0, 31, 32 or 63 and on the other 63 lanes
    (a) one-round walkers, (b) frames that never walk, (c) frames whose record is no candidate's.
    Last: 17 frames, one-round walkers and the 40-round one at the end.  meta: the slice's kind."""
    base = [rounds_frame(r, k) for k, r in enumerate(base_rounds())]
    slowest = base_rounds().index(MAX_ROUNDS)
    frames, verd, meta = list(base), [int(CAND[k % 3]) for k in range(SLICE)], ["base"] * SLICE
    for lane in EDGE_LANES:
        s = list(base)
        s[slowest], s[lane] = s[lane], s[slowest]
        frames += s
        verd += [int(CAND[(k + lane) % 3]) for k in range(SLICE)]
        meta += ["permuted"] * SLICE
    for kind in ("one_round", "never", "non_candidate"):
        for lane in EDGE_LANES:
            for k in range(SLICE):
                if k == lane:
                    frames.append(rounds_frame(MAX_ROUNDS, k))
                    verd.append(int(CAND[lane % 3]))
                elif kind == "one_round":
                    frames.append(rounds_frame(1, 64 * lane + k))
                    verd.append(int(CAND[k % 3]))
                elif kind == "never":
                    frames.append(never_walks(k + lane))
                    verd.append(int(CAND[k % 3]))
                else:
                    frames.append(rounds_frame(2 + (k + lane) % 36, k))
                    verd.append(int(OTHER[k % 3]))
                meta.append(kind)
    frames += [rounds_frame(1, 900 + k) for k in range(16)] + [rounds_frame(MAX_ROUNDS, 0)]
    verd += [int(CAND[k % 3]) for k in range(17)]
    meta += ["partial"] * 17
    return Case("rounds", frames, verdicts=verd, meta=meta)


# ----------------------------------------------------------------------- length_tests ---
OPT_SIZES = list(range(4, 44, 4))
LENGTH_KINDS = [2, 3, 4, 5, 8, 77]
# every length byte 0..42 (two past the largest O), and a few with the high bits set
LENGTH_BYTES = list(range(43)) + [127, 128, 129, 130, 255]
FILL = bytes([3, 3, 0x51]) * 14     # an option's value: window scales, so a walk that lands in it finds one


def length_frame(size: int, p: int, kind: int, ln: int) -> bytes:
    """`p` no-operations, then (kind, ln).  A length the rule takes: its value, then an MSS where
    four bytes are left, no-operations to O.  One it refuses: the MSS right behind the length byte
    where it fits, then the fill.  A skip by a wrong count or a walk that goes on shows."""
    v = (997 * size + 43 * p + ln) & 0xFFFF
    if ln >= 2 and p + ln <= size:
        left = size - p - ln
        body = NOP * p + bytes([kind, ln]) + FILL[:ln - 2] + (mss(v) + NOP * (left - 4) if left >= 4 else NOP * left)
    else:
        room = size - p - 2
        body = NOP * p + bytes([kind, ln]) + ((mss(v) + FILL)[:room] if room >= 4 else FILL[:room])
    return seg(body)


@functools.lru_cache(maxsize=None)
def length_tests(size: int) -> Case:
    """For one O: every p <= O - 2 behind p no-operations, every length byte of LENGTH_BYTES, every
    kind of LENGTH_KINDS (meta (O, p, kind, l)); and every kind at p = O - 1, where there is no
    length byte (l None).  The frames end with their options (at most 94 bytes)."""
    frames, meta = [], []
    for p in range(size - 1):
        for kind in LENGTH_KINDS:
            for ln in LENGTH_BYTES:
                frames.append(length_frame(size, p, kind, ln))
                meta.append((size, p, kind, ln))
    for kind in LENGTH_KINDS:
        frames.append(seg(NOP * (size - 1) + bytes([kind])))
        meta.append((size, size - 1, kind, None))
    # slices are not to be 48 length bytes of one (p, kind) after another
    order = (np.arange(len(frames)) * 101) % len(frames)
    assert np.gcd(101, len(frames)) == 1
    return Case(f"length_tests[{size}]", [frames[i] for i in order], meta=[meta[i] for i in order])


# -------------------------------------------------------------------------- sack_grid ---
def sack_grid() -> Case:
    """SACK with 1..4 blocks at every p where it fits, for every O (meta (O, blocks, p)); behind it
    an MSS where four bytes are left."""
    frames, meta = [], []
    for size in OPT_SIZES:
        for nb in (1, 2, 3, 4):
            ln = 2 + 8 * nb
            for p in range(size - ln + 1):
                left = size - p - ln
                frames.append(seg(NOP * p + sack(nb, (size << 16) | (p << 8) | nb)
                                  + (mss(0x3000 + p) + NOP * (left - 4) if left >= 4 else NOP * left)))
                meta.append((size, nb, p))
    return Case("sack_grid", frames, meta=meta)


# ---------------------------------------------------------------------- aligned_edges ---
def _more_options(room: int, k: int) -> bytes:
    out = b""
    while room - len(out) >= 4:
        out += mss(0x2000 + 16 * k + len(out))
    return out + NOP * (room - len(out))


def aligned_edges() -> Case:
    """meta ("bit", j): O = 12 with bit j of 01 01 08 0A flipped in option dword 0; ("exact", O):
    that dword first under O = 8..40 with a timestamp's value and MSS options behind it (O = 8: the
    timestamp does not fit); ("len", n): the aligned timestamp of O = 12 cut at len n = 54..70."""
    frames, meta = [], []
    word = int.from_bytes(cases.ALIGNED_TS, "little")
    for j in range(32):
        frames.append(seg((word ^ (1 << j)).to_bytes(4, "little") + bytes([0x71, j, 0x72, 0x73, 0x74, 0x75, 0x76, j]), 66 + j))
        meta.append(("bit", j))
    for size in range(8, 44, 4):
        body = (aligned_ts(0x77000000 + size, 0x78000000 + size) + _more_options(28, size))[:size]
        frames.append(seg(body, 54 + size + size % 7))
        meta.append(("exact", size))
    for n in range(54, 71):
        frames.append(seg(aligned_ts(0x79000000 + n, 0x7A000000 + n), n))
        meta.append(("len", n))
    return Case("aligned_edges", frames, meta=meta)


SETS = dict(len_grid=len_grid, len_grid_long=len_grid_long, verdicts=verdicts, rounds=rounds, sack_grid=sack_grid,
            aligned_edges=aligned_edges, **{f"length_tests[{size}]": functools.partial(length_tests, size) for size in OPT_SIZES})


@functools.lru_cache(maxsize=None)
def get(name: str) -> Case:
    return SETS[name]()


# ------------------------------------------------------------------------------- grid ---
POOL_FRAMES = tc.POOL_LINES        # 257, prime: a frame's slot never lines up with lanes or slices
SLOT_LINES = 2
GRID_SIZES = [255, 256, 257, 511, 512, 513, 769]
GRID_LARGE = (1 << 20) + 81
# 8 waves per SIMD, four SIMDs per CU, four waves per workgroup
RESIDENT_WORKGROUPS = 8


@functools.lru_cache(maxsize=None)
def grid_slots():
    """257 distinct frames of at most 128 bytes: the rounds base slice, the aligned edges and every
    37th frame of len_grid's grid."""
    seen, out = set(), []
    for f in get("rounds").frames[:SLICE] + get("aligned_edges").frames + get("len_grid").frames[LANE_BLOCK::37]:
        if len(f) <= SLOT_LINES * 64 and f not in seen:
            seen.add(f)
            out.append(f)
    assert len(out) >= POOL_FRAMES
    return out[:POOL_FRAMES]


class GridCase:
    """n frames addressed into a pool of 257 two-line slots: frame i is slot (101 i + seed) mod 257
    with that slot's length, under a seeded verdict 0..5."""

    def __init__(self, n: int, seed: int = 5):
        self.n, self.seed = n, seed
        self.slot = (101 * np.arange(n, dtype=np.int64) + seed) % POOL_FRAMES
        self.verdicts = np.random.default_rng(seed + n).integers(0, 6, n).astype(np.uint8)
        slots = grid_slots()
        self.slot_lens = np.array([len(f) for f in slots], np.int64)
        self.lens = self.slot_lens[self.slot].astype(np.uint16)
        self.off = (self.slot * SLOT_LINES).astype(np.uint32)

    def recs(self, rec_kind: int) -> np.ndarray:
        return tc.make_recs(self.verdicts, rec_kind, self.seed + rec_kind)

    def pool(self) -> np.ndarray:
        arena = poison(POOL_FRAMES * SLOT_LINES * 64).copy()
        _scatter(arena, np.arange(POOL_FRAMES) * SLOT_LINES * 64, grid_slots(), self.slot_lens)
        return arena

    def strided(self, slot0: int = 3):
        """(pool, (slot0, stride64)): frame i's slot copied to slot0 + i * 2."""
        arena = np.full((slot0 + self.n * SLOT_LINES) * 64, 0x08, np.uint8)
        arena[slot0 * 64:] = self.pool().reshape(POOL_FRAMES, -1)[self.slot].reshape(-1)
        return arena, (slot0, SLOT_LINES)

    @functools.cached_property
    def want(self) -> np.ndarray:
        per_slot = want(grid_slots(), np.zeros(POOL_FRAMES, np.uint8))
        out = per_slot[self.slot]
        out[~np.isin(self.verdicts, CAND)] = np.zeros(1, rxg.RX_OPT_DTYPE)[0]
        return out

    def frame(self, i: int) -> bytes:
        return grid_slots()[int(self.slot[i])]
