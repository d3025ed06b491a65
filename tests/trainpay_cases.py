"""Case sets for the train-payload tests (tests/test_trainpay_host.py, tests/test_gpu_trainpay.py):
small deterministic bursts, each a frame pool with crafted records, and the claim each makes
about the place it reaches (asserted on the model's output in test_trainpay_host.py).

A frame is random bytes -- also past its length, up to the end of its last 64-byte slot -- with
seq at 38..42 and the TCP header length in byte 46's high nibble; its payload is whatever random
bytes lie at 34 + header length."""
from dataclasses import dataclass, field

import numpy as np

import flowsum_cases as fc
import flowtrain_cases as ftc
import flowtrain_ref
import rxg
import trainpay_ref as ref

TILE = rxg.TRAIN_PAY_TILE                       # trains / segments per tile
ROUND = TILE * rxg.TRAIN_PAY_SCAN_TILES         # trains per round of the offset scan
ACK, FIN = 0x10, 0x01
OK = fc.OK


@dataclass
class Burst:
    name: str
    rec48: np.ndarray
    ntcb: int
    pool: np.ndarray
    off64: np.ndarray
    lens: np.ndarray
    cur: object = None                  # cur_seq array or None
    claims: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.rec48)

    def records(self, rec_kind):
        return np.ascontiguousarray(fc.as_kind(self.rec48, rec_kind)).view(np.uint8)

    def frames(self):
        return [self.pool[o * 64:o * 64 + ln].tobytes() for o, ln in zip(self.off64.tolist(), self.lens.tolist())]

    def strided(self):
        """(pool, slot0, stride64) with the same frames at a fixed stride, or None where that pool
        would be large."""
        s64 = (int(self.lens.max()) + 63) // 64 if self.n else 1
        if s64 * self.n > 1 << 16:
            return None
        rng = np.random.default_rng(99)
        pool = rng.integers(0, 256, (3 + self.n * s64) * 64, dtype=np.uint8)
        for i, (o, ln) in enumerate(zip(self.off64.tolist(), self.lens.tolist())):
            r = (ln + 63) // 64 * 64
            pool[(3 + i * s64) * 64:(3 + i * s64) * 64 + r] = self.pool[o * 64:o * 64 + r]
        return pool, 3, s64

    def trains(self, rec_kind=rxg.REC48):
        """The flow-train model's (order, trains, count) for this burst."""
        return flowtrain_ref.trains(self.records(rec_kind), rec_kind, self.ntcb,
                                    None if rec_kind == rxg.REC48 else self.frames(), 0, self.cur)


def build(name, rec48, ntcb, doff=5, lens=None, cur=None, shuffle=False, seed=0, claims=None):
    """doff: TCP header length in words per frame; lens: frame lengths (None: header + datalen,
    at least 54)."""
    n = len(rec48)
    rng = np.random.default_rng(seed + 1000)
    doff = np.broadcast_to(np.asarray(doff, np.int64), (n,))
    dl = np.maximum(rec48["c"]["datalen"].astype(np.int64), 0)
    if lens is None:
        lens = np.maximum(34 + 4 * doff + dl, 54)
    lens = np.broadcast_to(np.asarray(lens, np.int64), (n,)).copy()
    assert lens.max(initial=0) <= 65535
    slots = (lens + 63) // 64
    place = rng.permutation(n) if shuffle else np.arange(n)
    start = np.zeros(n, np.int64)
    start[place] = np.cumsum(slots[place]) - slots[place]
    off64 = (start + 2).astype(np.uint32)                  # two slots of other data in front
    pool = rng.integers(0, 256, (int(slots.sum()) + 4) * 64, dtype=np.uint8)
    base = off64.astype(np.int64) * 64
    seq = rec48["seq"].astype(np.int64)
    for k in range(4):
        pool[base + 38 + k] = (seq >> (8 * (3 - k))) & 0xFF
    pool[base + 46] = (doff << 4) | (pool[base + 46] & 0xF)
    curarr = None
    if cur is not None:
        curarr = np.zeros(ntcb, np.uint32)
        for t, v in cur.items():
            curarr[t] = v
    return Burst(name, rec48, ntcb, pool, off64, lens.astype(np.uint16), curarr, claims or {})


def chains(spec, seq0=None, seed=0):
    """spec: a list of (tcb, [datalen, ...]) contiguous chains, frames in that order."""
    rng = np.random.default_rng(seed)
    parts = []
    for q, (tcb, dls) in enumerate(spec):
        s0 = int(rng.integers(1, 1 << 31)) if seq0 is None else seq0[q]
        parts.append(ftc.chain(tcb, s0, dls))
    return np.concatenate(parts)


def shifts():
    """1. payload lengths 1..33 at every destination offset 0..15 (a segment of that many bytes in
    front, in the same train), TCP headers of 20, 24, 28, 32 and 60 bytes."""
    spec, doff, flow = [], [], 0
    for hl in (5, 6, 7, 8, 15):
        for lead in range(16):
            for ln in range(1, 34):
                dls = ([lead] if lead else []) + [ln]
                spec.append((flow, dls))
                doff += [hl] * len(dls)
                flow += 1
    return build("1: lengths 1..33 at offsets 0..15, five header lengths", chains(spec, seed=1), flow, doff=doff,
                 seed=1, claims={"trains": flow, "holes": 0, "offsets": 16})


def sets():
    out = [shifts()]
    out.append(build("2: forty 1-byte segments in one train, then a 17-byte train",
                     chains([(0, [1] * 40), (1, [17])], seed=2), 2, seed=2,
                     claims={"trains": 2, "holes": 0, "bytes": [40, 17], "pad": [8, 15]}))
    sizes = [1, 2, 64, 65, 256, 257, 1024, 1025]
    rng = np.random.default_rng(3)
    out.append(build("3: trains of 1 .. 1 025 segments", chains([(q, rng.integers(1, 40, k).tolist())
                                                                  for q, k in enumerate(sizes)], seed=3),
                     len(sizes), seed=3, claims={"trains": len(sizes), "nseg": sizes, "holes": 0}))
    a, b = ftc.chain(7, 5000, [13] * 150), ftc.chain(2, 90000, [29] * 150)
    alt = np.empty(300, a.dtype)
    alt[0::2], alt[1::2] = a, b
    out.append(build("3: two flows alternating", alt, 8, seed=4, cur={7: 5000},
                     claims={"trains": 2, "holes": 0, "reordered": True}))
    out.append(build("4: one train of 4 096 segments", ftc.chain(0, 777, rng.integers(1, 20, 4096)), 1, seed=5,
                     claims={"trains": 1, "nseg": [4096], "holes": 0}))
    out.append(build("4: 4 096 trains of one segment", ftc.craft(np.arange(4096)[::-1].copy(), rng.integers(1, 1 << 31, 4096),
                                                                 rng.integers(1, 20, 4096)), 4096, seed=6,
                     claims={"trains": 4096, "holes": 0}))
    for n in (ROUND - 1, ROUND, ROUND + 1):
        out.append(build(f"5: {n} single-segment trains of 1 byte (a scan round is {ROUND} trains)",
                         ftc.craft(np.arange(n), np.arange(n) * 7 + 1, 1), n, seed=n,
                         claims={"trains": n, "holes": 0, "used": 16 * n}))
    # 6. holes in the middle of a train of five 100-byte segments (each set: the third is the hole)
    five = lambda: ftc.chain(1, 4000, [100] * 5)                                         # noqa: E731
    out.append(build("6: a payload past len", five(), 2, lens=[154, 154, 153, 154, 154], seed=7,
                     claims={"trains": 1, "holes": 1, "hole_at": 2}))
    r = five()
    c = r["c"]
    c["flags"][2] = OK | rxg.F_TRUNC
    r["c"] = c
    out.append(build("6: a TRUNC record", r, 2, seed=8, claims={"trains": 1, "holes": 1, "hole_at": 2}))
    for ln in (53, 54, 55):
        out.append(build(f"6: a frame cut at {ln} bytes", five(), 2, lens=[154, 154, ln, 154, 154], seed=ln,
                         claims={"trains": 1, "holes": 1, "hole_at": 2}))
    out.append(build("6: a frame cut at 46 bytes (byte 46 unreadable), 1-byte payload at header length 0",
                     ftc.chain(1, 4000, [100, 1, 100]), 2, doff=[5, 0, 5], lens=[154, 46, 154], seed=9,
                     claims={"trains": 1, "holes": 1, "hole_at": 1}))
    # 8. sequence-space edges
    out.append(build("8: a WRAP segment between two trains", ftc.chain(1, 0xFFFFFFF0 - 10, [10, 0x20, 10]), 2,
                     cur={1: 0xFFFFFFF0 - 10}, seed=10, claims={"trains": 3, "holes": 0, "wraps": 1}))
    out.append(build("8: a train ending at 0xFFFFFFFF", np.concatenate([ftc.chain(1, 0xFFFFFFFF - 30, [10, 20]),
                                                                          ftc.chain(1, 0, [5])]), 2,
                     cur={1: 0xFFFFFFFF - 30}, seed=11, claims={"trains": 2, "holes": 0, "heads": 1}))
    # 9. one 65 481-byte segment between 1-byte segments, the pool shuffled
    out.append(build("9: a 65 481-byte segment between 1-byte segments", ftc.chain(3, 10, [1] * 20 + [65481] + [1] * 20), 4,
                     shuffle=True, seed=12, claims={"trains": 1, "holes": 0, "maxlen": 0xFFFF}))
    # 7. the set the caps are cut on: six flows, cur_seq matching three of them
    spec = [(q, np.random.default_rng(20 + q).integers(1, 300, 3 + q).tolist()) for q in range(6)]
    seq0 = [1000 * (q + 1) for q in range(6)]
    out.append(build("7: six trains, three of them HEAD", chains(spec, seq0), 6, cur={0: 1000, 2: 3000, 3: 4001, 5: 6000},
                     seed=13, claims={"trains": 6, "holes": 0, "heads": 3}))
    return out


BY_NAME = None


def by_name(prefix):
    global BY_NAME
    if BY_NAME is None:
        BY_NAME = sets()
    return next(b for b in BY_NAME if b.name.startswith(prefix))


def all_sets():
    by_name("1")
    return BY_NAME


def model(b, rec_kind=rxg.REC48, cap_seg=None, cap_trains=None, flags=0, arena_cap=None, fill=0xA5, pool=None,
          off64=None, want_msgs=True, want_tmsgs=True, slack=64):
    """The model's answer for burst b: (arena of arena_cap + slack bytes prefilled with `fill`,
    msgs, tmsgs, used), and the (order, trains, count) it was given."""
    order, trains, count = b.trains(rec_kind)
    cap_seg = len(order) if cap_seg is None else cap_seg
    cap_trains = len(trains) if cap_trains is None else cap_trains
    full = int(ref.pad16(trains["bytes"].astype(np.int64)).sum())
    arena_cap = full if arena_cap is None else arena_cap
    before = np.full(min(arena_cap, full) + slack, fill, np.uint8)
    got = ref.gather(b.pool if pool is None else pool, b.off64 if off64 is None else off64, b.lens, b.records(rec_kind),
                     rec_kind, order, trains, count, cap_seg, cap_trains, flags, before, arena_cap, want_msgs, want_tmsgs)
    return got, (order, trains, count, cap_seg, cap_trains, arena_cap)
