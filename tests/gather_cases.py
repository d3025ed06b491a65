"""Deterministic payload-gather cases (pg_gather, csrc/rxg_payload.hip): payload lengths and source
shifts at every tail and chunk edge, a payload's chunks placed on every lane of the wave's run and
across its 64-, 128- and 256-chunk marks, jumbo payloads, wave and workgroup occupancy edges, a
sparse burst of seventy workgroups, and the candidate rule stated case by case.

Every builder is seeded and returns (rows, frames) for pktgen.table_arrays / pktgen.pack_arena
(occupancy_sets: a dict of them).  Frames are pktgen.frame on one ESTABLISHED flow, among fillers
that are no candidates: a 54-byte pure ACK, and an IPv4 frame of another protocol that carries
data.  (A TCP segment with a bad checksum that carries data IS a candidate -- the gather does not
look at the checksums, oracle/payload.py -- so it is one of rule_edges' cases, not a filler.)
meant(...) names the frames each builder means as candidates; the host test checks that against
the oracle.

layout() restates where the kernel puts a payload's 16-byte chunks in a wave's run; it is used
only to prove that the sets cover what they claim (tests/test_gather_cases_host.py).
"""
from __future__ import annotations

import functools
import random

import numpy as np

import pktgen
from rxspan_cases import rewrite_checksums

WAVE, WORKGROUP = 64, 1024        # frames per wave and per workgroup of pg_gather
MARKS = (64, 128, 256)            # run chunks: one round, one set of rounds, two sets in flight
MAX_FRAME = 65535                 # a frame's length is 16 bits
MAX_PAYLOAD = MAX_FRAME - 54      # with 20-byte IPv4 and TCP headers
OCC_N = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 3 * 1024 + 1)
OCC_LENGTHS = (1, 15, 16, 17, 100, 1446)
EXACT_T = (1, 63, 64, 65, 128, 129, 256, 257)
SPARSE_N = 70 * 1024 + 5

DST = pktgen.ip4(192, 168, 78, 2)
SRC = pktgen.ip4(10, 0, 0, 1)
# slot 0: the flow every payload belongs to; slot 1: a listener (rule_edges' resets)
ROWS = [(80, 1024, pktgen.raw_of_host(DST), SRC, pktgen.ESTABLISHED),
        (8080, 0, pktgen.raw_of_host(DST), 0, pktgen.LISTENING)]

ACK_FILLER = pktgen.frame(sport=1024)
DROP_FILLER = pktgen.frame(sport=1024, proto=17, payload=bytes(range(1, 41)))
FILLERS = (ACK_FILLER, DROP_FILLER)
assert len(ACK_FILLER) == 54


def chunks(length: int) -> int:
    return (int(length) + 15) // 16


def shift_of(f: bytes) -> int:
    """The payload's source offset modulo 16 (frames start 64-byte aligned)."""
    return (34 + 4 * (f[46] >> 4)) % 16


def own_bytes(f: bytes, length: int) -> bytes:
    """The bytes the hand-off takes from a frame: `length` bytes at 34 + 4 * data_off."""
    start = 34 + 4 * (f[46] >> 4)
    return bytes(f[start:start + length])


def layout(lens):
    """lens[i]: frame i's payload length, 0 for no candidate.  Within each aligned group of 64
    consecutive frames a candidate's first run chunk is the sum of ceil(L / 16) over the group's
    earlier candidates, its last one the first + ceil(L / 16) - 1.  Returns (first, last, T): per
    frame (-1: no candidate), and each group's total run."""
    n = len(lens)
    first = np.full(n, -1, dtype=np.int64)
    last = np.full(n, -1, dtype=np.int64)
    totals = []
    for g in range(0, n, WAVE):
        run = 0
        for i in range(g, min(g + WAVE, n)):
            if lens[i]:
                first[i], last[i] = run, run + chunks(lens[i]) - 1
                run += chunks(lens[i])
        totals.append(run)
    return first, last, np.array(totals, dtype=np.int64)


def aggregates(lens):
    """Chunks per workgroup of 1 024 frames: the value each workgroup publishes."""
    c = (np.asarray(lens, dtype=np.int64) + 15) // 16
    return np.array([int(c[g:g + WORKGROUP].sum()) for g in range(0, len(c), WORKGROUP)], dtype=np.int64)


def data_frame(rng, length: int, doff: int = 5, **kw) -> bytes:
    """A segment of the ESTABLISHED flow: random payload whose last byte is not zero (a tail
    byte lost to the mask shows), random option bytes."""
    body = rng.randbytes(length - 1) + bytes([rng.randrange(1, 256)]) if length else b""
    kw.setdefault("sport", 1024)
    kw.setdefault("flags", 0x18)
    return pktgen.frame(doff=doff, seq=rng.getrandbits(32), ack=rng.getrandbits(32), payload=body,
                        tcp_opts=rng.randbytes(max(0, doff - 5) * 4), **kw)


def _public(built):
    rows, frames = built[0], built[1]
    return list(rows), list(frames)


# -------------------------------------------------------------------- shift_tail_grid ---

def shift_tail_lengths() -> list[int]:
    ks = (8, 62, 63, 64, 90, 127, 128, 129, 255, 256, 257)
    return list(range(1, 81)) + [16 * k + d for k in ks for d in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def _shift_tail_grid():
    rng = random.Random(0x6A01)
    frames = [data_frame(rng, length, doff) for length in shift_tail_lengths() for doff in range(5, 16)]
    return tuple(ROWS), tuple(frames), tuple([True] * len(frames))


def shift_tail_grid():
    """Every payload length 1..80 and 16k - 1, 16k, 16k + 1 around the one- and two-set marks, at
    every data_off 5..15: all four source shifts (6, 10, 14, 2) times all sixteen tails."""
    return _public(_shift_tail_grid())


# ------------------------------------------------------------------ run_position_grid ---

def _length_of(rng, nch: int) -> int:
    return 16 * nch - rng.randrange(16)


def _leads(rng, nch: int) -> list[bytes]:
    """Payloads that fill `nch` run chunks before a probe: one, or two that share them."""
    if nch == 0:
        return []
    parts = [nch]
    if nch >= 2 and rng.random() < 0.5:
        a = rng.randrange(1, nch)
        parts = [a, nch - a]
    return [data_frame(rng, _length_of(rng, p), rng.choice((5, 6, 7, 8))) for p in parts]


def _batch(rng, cands):
    """64 frames: the candidates in order on random lanes, fillers on the others.  Returns the
    frames and each candidate's lane."""
    assert len(cands) <= WAVE
    lanes = sorted(rng.sample(range(WAVE), len(cands)))
    out = [FILLERS[rng.randrange(2)] for _ in range(WAVE)]
    for lane, f in zip(lanes, cands):
        out[lane] = f
    return out, lanes


@functools.lru_cache(maxsize=None)
def _run_position_grid():
    rng = random.Random(0x6A02)
    frames, probes = [], []

    def add(lead_chunks, probe_chunks, trailer):
        lead = _leads(rng, lead_chunks)
        probe = data_frame(rng, _length_of(rng, probe_chunks), rng.choice((5, 6, 7, 8)))
        tail = [data_frame(rng, rng.randrange(1, 17))] if trailer else []
        batch, lanes = _batch(rng, lead + [probe] + tail)
        probes.append(len(frames) + lanes[len(lead)])
        frames.extend(batch)

    # a three-chunk probe starting on every lane: its last chunk is on lanes 2..63, 0, 1
    for s in range(WAVE):
        add(s, 3, trailer=bool(s & 1))
    for m in MARKS:
        add(m - 2, 5, True)     # starts before the mark, ends after it
        add(m, 2, True)         # starts exactly at it
        add(m - 3, 3, True)     # ends exactly before it (the trailer then starts at it)
        add(m - 3, 3, False)    # ... and is the run's end
    add(54, 300, True)          # one payload across all three marks
    for t in EXACT_T:           # the batch's whole run
        if t == 1:
            add(0, 1, False)
        else:
            add(t - 2, 2, False)
    batch, _ = _batch(rng, [data_frame(rng, 1, rng.choice((5, 6, 7, 8))) for _ in range(WAVE)])
    frames.extend(batch)
    batch, lanes = _batch(rng, [data_frame(rng, MAX_PAYLOAD)])
    probes.append(len(frames) + lanes[0])
    frames.extend(batch)
    assert len(frames) % WAVE == 0
    return tuple(ROWS), tuple(frames), tuple(f not in FILLERS for f in frames), tuple(probes)


def run_position_grid():
    """Batches of 64 frames in which leading payloads of chosen length place a probe payload."""
    return _public(_run_position_grid())


def run_position_probes() -> list[int]:
    """The probes' frame indices in run_position_grid()."""
    return list(_run_position_grid()[3])


# ---------------------------------------------------------------------- jumbo_lengths ---

def jumbo_cells() -> list[tuple[int, int]]:
    """(payload length, data_off).  At data_off 15 the largest payload is the largest that a
    65 535-byte frame holds behind a 60-byte TCP header."""
    return [(4095, 5), (4096, 5), (4097, 5), (9000, 5), (MAX_PAYLOAD, 5), (9000, 15), (MAX_PAYLOAD - 40, 15)]


@functools.lru_cache(maxsize=None)
def _jumbo_lengths():
    rng = random.Random(0x6A03)
    frames = []
    pairs = [(data_frame(rng, length, doff), data_frame(rng, 1, doff)) for length, doff in jumbo_cells()]
    assert max(len(j) for j, _ in pairs) == MAX_FRAME
    for pair in pairs:                       # a batch of its own for each jumbo and its follower
        lane = rng.randrange(WAVE - 1)
        batch = [FILLERS[rng.randrange(2)] for _ in range(WAVE)]
        batch[lane:lane + 2] = pair
        frames.extend(batch)
    batch = [FILLERS[rng.randrange(2)] for _ in range(WAVE)]
    for k, pair in enumerate(pairs):         # and all of them in one batch
        batch[3 + 8 * k:5 + 8 * k] = pair
    frames.extend(batch)
    return tuple(ROWS), tuple(frames), tuple(f not in FILLERS for f in frames)


def jumbo_lengths():
    """Payloads of 4 095, 4 096, 4 097, 9 000 and 65 481 bytes, the two largest again at data_off
    15, each followed by a one-byte payload in the same batch."""
    return _public(_jumbo_lengths())


# --------------------------------------------------------------------- occupancy_sets ---

@functools.lru_cache(maxsize=None)
def _occupancy_sets():
    rng = random.Random(0x6A04)
    pool = [data_frame(rng, length, doff) for length in OCC_LENGTHS for doff in (5, 5, 6, 7, 8)]
    sets = {}

    def put(name, n, want):
        want = [bool(w) for w in want]
        frames = [pool[rng.randrange(len(pool))] if w else FILLERS[i & 1] for i, w in enumerate(want)]
        sets[f"n{n}_{name}"] = (tuple(ROWS), tuple(frames), tuple(want))

    for n in OCC_N:
        idx = range(n)
        nwg = (n + WORKGROUP - 1) // WORKGROUP
        nwave = (n + WAVE - 1) // WAVE
        half = [rng.random() < 0.5 for _ in idx]
        put("lane0", n, [i % WAVE == 0 for i in idx])
        put("lane63", n, [i % WAVE == 63 for i in idx])     # (n of 1 and 63: no candidate at all)
        put("single_first", n, [i == 0 for i in idx])
        put("single_last", n, [i == n - 1 for i in idx])
        if n > WORKGROUP:
            put("single_1024", n, [i == WORKGROUP for i in idx])
        put("one_wave", n, [i // WAVE == nwave // 2 for i in idx])
        if nwg >= 2:
            put("first_wg_empty", n, [i >= WORKGROUP and (half[i] or i == n - 1) for i in idx])
            put("last_wg_empty", n, [i // WORKGROUP != nwg - 1 and (half[i] or i == 0) for i in idx])
        if nwg >= 3:
            mid = (nwg - 1) // 2
            put("middle_wg_empty", n, [i // WORKGROUP != mid and (half[i] or i in (0, n - 1)) for i in idx])
    return sets


def occupancy_sets():
    """{name: (rows, frames)} for every n of OCC_N: candidates only on lane 0 of each wave, only on
    lane 63, a single candidate (first, last, frame 1024), every wave but one empty, the first, the
    middle and the last workgroup empty."""
    return {name: _public(s) for name, s in _occupancy_sets().items()}


def occupancy_names(n: int) -> list[str]:
    return [name for name in _occupancy_sets() if name.startswith(f"n{n}_")]


# ------------------------------------------------------------- sparse_many_workgroups ---

@functools.lru_cache(maxsize=None)
def _sparse_many_workgroups(seed: int):
    rng = random.Random(0x6A05 + seed)
    lengths = [1, 15, 16, 17, 100, 536, 1446, 1460] + [rng.randrange(1, 1461) for _ in range(54)]
    pool = [data_frame(rng, length, rng.choice((5, 5, 6, 7, 8))) for length in lengths]
    assert len(set(pool)) + len(FILLERS) <= 64
    nwg = (SPARSE_N + WORKGROUP - 1) // WORKGROUP
    empty = set(rng.sample(range(2, nwg - 3), 5))
    empty.add(min(empty) + 1)                       # two empty workgroups in a row
    density = [0.0 if g in empty else rng.choice((1 / 80, 1 / 40, 1 / 40, 1 / 20)) for g in range(nwg)]
    want = [rng.random() < density[i // WORKGROUP] for i in range(SPARSE_N)]
    want[SPARSE_N - 1] = True                       # the last, five-frame workgroup has one
    frames = [pool[rng.randrange(len(pool))] if w else FILLERS[i & 1] for i, w in enumerate(want)]
    return tuple(ROWS), tuple(frames), tuple(want), tuple(sorted(empty))


def sparse_many_workgroups(seed: int):
    """70 * 1024 + 5 frames of at most 64 distinct frame objects, about one in 40 a candidate,
    workgroups of different density and six interior ones with none: predecessors at distance 64
    and more for the last workgroups' look-back."""
    return _public(_sparse_many_workgroups(seed))


def sparse_empty_workgroups(seed: int) -> list[int]:
    return list(_sparse_many_workgroups(seed)[3])


# ------------------------------------------------------------------------- rule_edges ---

RULE_KINDS = {  # name: (pktgen.frame arguments, the verdict the oracle must give)
    "dispatch": (dict(sport=1024, dport=80), 0),
    "rst_nopcb": (dict(sport=2000, dport=81), 1),
    "rst_listen_nonsyn": (dict(sport=2000, dport=8080), 2),
    "drop_nontcp": (dict(sport=1024, dport=80, proto=17), 3),
}


@functools.lru_cache(maxsize=None)
def _rule_edges():
    rng = random.Random(0x6A06)
    frames, kinds = [], []

    def patched(f, at, value):
        b = bytearray(f)
        b[at:at + len(value)] = value
        return rewrite_checksums(b)

    for kind, (kw, _verdict) in RULE_KINDS.items():
        whole = data_frame(rng, 33, **kw)
        long_ = data_frame(rng, 100, **kw)
        tl = int.from_bytes(whole[16:18], "big")
        cases = [
            data_frame(rng, 0, **kw),                                # datalen 0
            data_frame(rng, 1, **kw),                                # datalen 1
            whole,                                                   # ends at the frame's end
            patched(whole, 16, (tl + 1).to_bytes(2, "big")),         # one byte past it
            patched(whole, 16, (65535).to_bytes(2, "big")),          # far past it
            long_[:53], long_[:40],                                  # truncated records
            patched(long_, 14, b"\x46"), patched(long_, 14, b"\x4f"),  # IHL 6 and 15, data_off 5
            data_frame(rng, 40, valid_tcp=False, **kw),              # a bad TCP checksum
        ]
        cases += [data_frame(rng, 40, doff=d, **kw) for d in range(5)]  # data_off 0..4
        frames += cases
        kinds += [kind] * len(cases)
    return tuple(ROWS), tuple(frames), tuple(kinds)


def rule_edges():
    """For each verdict that gathers and for a dropped frame: datalen 0 and 1, a payload ending at
    the frame's end and past it, truncated records, IHL 6 and 15, data_off 0..4, a bad checksum.
    Which of them are candidates is the oracle's to say."""
    return _public(_rule_edges())


def rule_edge_kinds() -> list[str]:
    return list(_rule_edges()[2])


# ------------------------------------------------------------------- a set, answered ---

class Case:
    """A set packed once with the oracle's answer: its records, and oracle.payload.gather on them
    (expect(cap); full: the bytes the burst needs).  Shared by tests, left unchanged."""

    def __init__(self, rows, frames):
        import oracle
        self.frames = frames
        self.n = len(frames)
        self.arena, self.off, self.lens = pktgen.pack_arena(frames)
        self.tcb, self.live = pktgen.table_arrays(rows)
        self.exp, _ = oracle.rx_batch(self.arena, self.off, self.lens, self.tcb, self.live)
        for a in (self.arena, self.off, self.lens, self.exp):
            a.setflags(write=False)
        self._gathers = {}
        self.msgs, self.bytes, self.full = self.expect(1 << 40)

    def expect(self, cap: int):
        """(msgs, the gathered messages' bytes, bytes needed) at an arena capacity."""
        from oracle import payload as opl
        if cap not in self._gathers:
            g = opl.gather(self.frames, self.exp["c"], cap)
            for a in g[:2]:
                a.setflags(write=False)
            self._gathers[cap] = g
        return self._gathers[cap]


# ------------------------------------------------------------------------------ meant ---

def meant(name: str, *args):
    """Per frame, whether the builder means it as a candidate (occupancy_sets: {name: ...})."""
    if name == "occupancy_sets":
        return {k: list(s[2]) for k, s in _occupancy_sets().items()}
    built = {"shift_tail_grid": _shift_tail_grid, "run_position_grid": _run_position_grid,
             "jumbo_lengths": _jumbo_lengths, "sparse_many_workgroups": _sparse_many_workgroups}[name](*args)
    return list(built[2])
