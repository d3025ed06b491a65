"""Deterministic cases for the device reset build (rxg_tx_reset_dev, csrc/rxg_txreset.hip): batches
that put the slice-count scan past its first lanes, waves and rounds, a slice's reset count on
every edge of the build pass's 16-reset rounds, `cap` inside a slice, every offender length at
the edges of the 16-byte chunks, and the checksum corners.

The call is a pure function of its arguments (include/rxg.h), so nothing here is a real burst:
the records are written in the documented layouts with every bit outside the verdict field
random (make_recs), and off64 points the frames of a batch of any size at a pool of a few hundred
64-byte lines.  A reset depends on its offender's line only, so the lines are seeded random
bytes, no valid TCP.

build_fast is a vectorised model with txreset_ref.build's contract (ref.build loops in Python per
reset, too slow for the 10^5 resets of the scan sizes); tests/test_txreset_cases_host.py pins it
to ref.build byte for byte and holds every claim made below against the masks themselves.
"""
from __future__ import annotations

import struct

import numpy as np

import oracle
import rxg
import txreset_ref as ref

# csrc/rxg_txreset.hip: tx_reset_count and tx_reset_build take a wave per 64-frame slice (:110,
# :226 "i = s * 64u + lane"); tx_reset_scan is one workgroup of kScanLanes = 1024 lanes with
# kScanPer = 16 entries each (:119), so a wave of 64 lanes covers 64 * 16 entries and a round of
# the loop kScanLanes * kScanPer (:125); tx_reset_build handles 16 resets per round (:244).
SLICE = 64
SCAN_PER = 16
SCAN_WAVE = 64 * 16
SCAN_ROUND = 1024 * 16
BUILD_ROUND = 16

GUARD = 8
MAC = bytes([0x02, 0xAB, 0xCD, 0xEF, 0x01, 0x99])
RST = np.array(ref.RST_VERDICTS, dtype=np.uint8)
OTHER = np.array([rxg.V_DISPATCH, rxg.V_DROP_NONTCP, rxg.V_ARP, rxg.V_DROP_L2], dtype=np.uint8)
assert sorted(RST.tolist() + OTHER.tolist()) == list(range(6))


# ------------------------------------------------------------------------------ records ---
def make_recs(verdicts, rec_kind: int, rng) -> np.ndarray:
    """u8[n * rec_kind]: rxg_rec8 / rxg_rec16 / rxg_rec48 records that carry `verdicts` (the six
    defined values) and random bits everywhere else: for REC8 bits 0-23 and 27-31 of w0 and all
    of w1, for REC16 / REC48 every byte but byte 8."""
    v = np.asarray(verdicts, dtype=np.uint8)
    assert v.size == 0 or int(v.max()) <= 5
    rng = np.random.default_rng(rng)
    if rec_kind == rxg.REC8:
        w = rng.integers(0, 1 << 32, size=(v.size, 2), dtype=np.uint64).astype(np.uint32)
        w[:, 0] = (w[:, 0] & ~np.uint32(7 << 24)) | (v.astype(np.uint32) << 24)
        return np.ascontiguousarray(w).view(np.uint8).reshape(-1)
    assert rec_kind in (rxg.REC16, rxg.REC48)
    r = rng.integers(0, 256, size=(v.size, rec_kind), dtype=np.uint8)
    r[:, 8] = v
    return r.reshape(-1)


def verdict_of(recs, rec_kind: int) -> np.ndarray:
    """The verdicts of records of any of the three kinds (raw bytes or a structured array)."""
    b = np.ascontiguousarray(recs).view(np.uint8).reshape(-1, rec_kind)
    if rec_kind == rxg.REC8:
        return ((np.ascontiguousarray(b[:, :4]).view("<u4")[:, 0] >> 24) & 7).astype(np.uint8)
    return b[:, 8].copy()


def verdicts_for(mask, rng) -> np.ndarray:
    """Verdicts whose RST frames are exactly `mask`: both RST verdicts and all four others."""
    mask = np.asarray(mask, dtype=bool)
    rng = np.random.default_rng(rng)
    return np.where(mask, RST[rng.integers(0, 2, mask.size)], OTHER[rng.integers(0, 4, mask.size)]).astype(np.uint8)


# -------------------------------------------------------------------------------- model ---
def build_fast(pool, off64, lens, verdicts, ip_id0, src_mac, cap):
    """txreset_ref.build's contract, vectorised: (out u8[min(count, cap) * 64], idx u32[..], count).
    Selects the RST frames in packet order, reads each one's first line with the bytes at and
    past len as zero, places the fields of txreset_ref.reset_unsummed, and leaves the two
    checksums to oracle.tx_batch."""
    pool = np.asarray(pool, dtype=np.uint8).reshape(-1)
    sel = np.nonzero(np.isin(np.asarray(verdicts), RST))[0]
    count = int(sel.size)
    sel = sel[:max(0, min(count, int(cap)))]
    m = int(sel.size)
    col = np.arange(64)
    inb = pool[np.asarray(off64, dtype=np.int64)[sel, None] * 64 + col]
    inb = np.where(col[None, :] < np.minimum(np.asarray(lens, dtype=np.int64)[sel], 64)[:, None], inb, 0).astype(np.uint8)
    ids = (int(ip_id0) + np.arange(m)) & 0xFFFF
    f = np.zeros((m, 64), dtype=np.uint8)
    f[:, 0:6] = inb[:, 6:12]
    f[:, 6:12] = np.frombuffer(bytes(src_mac), np.uint8)
    f[:, 12], f[:, 13] = 0x08, 0x00
    f[:, 14] = 0x45
    f[:, 17] = 40
    f[:, 18], f[:, 19] = ids & 0xFF, ids >> 8
    f[:, 22], f[:, 23] = 127, 6
    f[:, 26:30] = inb[:, 30:34]
    f[:, 30:34] = inb[:, 26:30]
    f[:, 34:36] = inb[:, 36:38]
    f[:, 36:38] = inb[:, 34:36]
    f[:, 38:42] = inb[:, 42:46]
    f[:, 46], f[:, 47] = 0x50, rxg.TCP_FLAG_RST
    f[:, 48], f[:, 49] = 12000 & 0xFF, 12000 >> 8
    out = f.reshape(-1)
    if m:
        out = oracle.tx_batch(out, np.arange(m, dtype=np.uint32), np.full(m, 54, np.uint16))
    return out, sel.astype(np.uint32), count


# --------------------------------------------------------------------------------- pool ---
POOL_LINES = 257   # prime: the slot a frame reuses never lines up with slices, lanes or rounds


def offender_pool() -> np.ndarray:
    """u8[257 * 64]: seeded random lines."""
    return np.random.default_rng(257).integers(0, 256, POOL_LINES * 64, dtype=np.uint8)


class Case:
    """One call's inputs.  pool: the frame pool (u8, whole lines), dev_pool: what the device is
    given where that differs (the length set's poisoned copy); off / lens per frame; mask: the
    frames that get a reset; verdicts: what the records carry."""

    def __init__(self, pool, off, lens, mask, seed, dev_pool=None, ip_id0=0, named=None):
        self.pool, self.dev_pool = pool, pool if dev_pool is None else dev_pool
        self.off, self.lens = np.asarray(off, np.uint32), np.asarray(lens, np.uint16)
        self.mask = np.asarray(mask, dtype=bool)
        self.n, self.seed, self.ip_id0, self.named = self.mask.size, seed, ip_id0, named or {}
        self.verdicts = verdicts_for(self.mask, seed)
        self.count = int(self.mask.sum())

    def recs(self, rec_kind):
        return make_recs(self.verdicts, rec_kind, self.seed + rec_kind)

    def want(self, cap, ip_id0=None, src_mac=MAC):
        return build_fast(self.pool, self.off, self.lens, self.verdicts, self.ip_id0 if ip_id0 is None else ip_id0,
                          src_mac, cap)

    def strided(self, slot0, stride64):
        """The same frames laid out at slot0 + i * stride64 in a pool of their own."""
        off = (slot0 + np.arange(self.n) * stride64).astype(np.uint32)
        pool = np.full((slot0 + max(self.n, 1) * stride64) * 64, 0x5A, np.uint8)
        pool.reshape(-1, 64)[off] = self.pool.reshape(-1, 64)[self.off]
        return Case(pool, off, self.lens, self.mask, self.seed, ip_id0=self.ip_id0)


SCAN_LENS = np.array([0, 20, 53, 54, 60, 64, 65, 1514], dtype=np.uint16)


def pooled(mask, seed, lens=None) -> Case:
    """Frame i at pool line (101 * i + seed) mod 257, its length a seeded pick of SCAN_LENS."""
    mask = np.asarray(mask, dtype=bool)
    off = (101 * np.arange(mask.size, dtype=np.int64) + seed) % POOL_LINES
    if lens is None:
        lens = SCAN_LENS[np.random.default_rng(seed + 1).integers(0, len(SCAN_LENS), mask.size)]
    return Case(offender_pool(), off, lens, mask, seed)


# ---------------------------------------------------------------------------- scan sizes ---
SCAN_NSLICES = [15, 16, 17, 1023, 1024, 1025, 16383, 16384, 16385, 16384 + 1025, 2 * 16384 + 17]
# the chance of a count of 0, 1, 2, 3, 5, 16, 17 on a slice that is not forced: mean 0.33
FREE_COUNTS = np.array([0, 1, 2, 3, 5, 16, 17])
FREE_P = np.array([0.88, 0.06, 0.03, 0.015, 0.007, 0.004, 0.004])
FREE_MEAN_MAX = 0.5


def forced_counts(nslices: int) -> dict:
    """slice -> 64 on the first and 1 on the last slice of every 16-entry lane group of the
    scan, which are also the first and last slices of its 1024-entry waves and 16 384-entry
    rounds, as far as they fall inside nslices."""
    f = {s: 64 for s in range(0, nslices, SCAN_PER)}
    f.update({s: 1 for s in range(SCAN_PER - 1, nslices, SCAN_PER)})
    return f


def slice_counts(nslices: int, seed: int) -> np.ndarray:
    """Per-slice reset counts: forced_counts where it says, a seeded pick of FREE_COUNTS elsewhere.

    The forced slices alone come to (64 + 1) / 16 = 4.06 resets per slice, so a mean of 4 over
    all slices cannot hold with them in place; what holds, from 1 023 slices up (below that the
    few free slices are too small a sample), is a mean of at most FREE_MEAN_MAX on the slices
    that are not forced and 4.5 over all, and under 10 MB of resets in the largest case."""
    c = FREE_COUNTS[np.random.default_rng(seed).choice(len(FREE_COUNTS), size=nslices, p=FREE_P)]
    c[-1] = max(c[-1], 1)       # the batch's last slice always holds a reset
    for s, v in forced_counts(nslices).items():
        c[s] = v
    return c.astype(np.int64)


def mask_of(counts, n: int, seed: int) -> np.ndarray:
    """bool[n]: slice s has min(counts[s], its frames) resets on seeded lanes."""
    counts = np.asarray(counts, dtype=np.int64)
    nslices = len(counts)
    assert (nslices - 1) * SLICE < n <= nslices * SLICE
    key = np.random.default_rng(seed + 7).random((nslices, SLICE))
    key[-1, n - (nslices - 1) * SLICE:] = 2.0        # lanes past n come last
    rank = np.argsort(np.argsort(key, axis=1), axis=1)
    return (rank < counts[:, None]).reshape(-1)[:n]


def scan_n(nslices: int):
    """The two batch sizes of a scan size: whole slices, and a last slice of one frame."""
    return (SLICE * nslices, SLICE * nslices - (SLICE - 1))


def scan_case(nslices: int, n: int) -> Case:
    seed = 9000 + nslices
    return pooled(mask_of(slice_counts(nslices, seed), n, seed), seed)


def flood_case(nslices: int) -> Case:
    """Every frame a reset: what leaves the largest prefix sums behind in the slice counts."""
    return pooled(np.ones(SLICE * nslices, dtype=bool), 77)


STALE_FIRST = 16385
STALE_THEN = (17, 1025, 15)

# ---------------------------------------------------------------------------- rank cases ---
RANK_COUNTS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
HOLES = [0, 31, 32, 63]


def spread_lanes(count: int) -> np.ndarray:
    """`count` lanes spread over the slice, first and last lane among them from 2 up."""
    return np.unique(np.round(np.linspace(0, SLICE - 1, count)).astype(int)) if count > 1 else np.array([29])


def rank_cases() -> dict:
    """name -> Case.  low / high / spread: a slice for every count of RANK_COUNTS, the resets on
    its lowest lanes, its highest lanes, spread; holes: four slices of 63 resets, lane 0, 31, 32
    or 63 missing; single: 64 slices with one reset, slice L's on lane L; last1 / last63: a
    partial last slice of 1 and of 63 frames with the reset on its last frame."""
    out = {}
    for name in ("low", "high", "spread"):
        m = np.zeros((len(RANK_COUNTS), SLICE), dtype=bool)
        for s, c in enumerate(RANK_COUNTS):
            lanes = np.arange(c) if name == "low" else np.arange(SLICE - c, SLICE) if name == "high" else spread_lanes(c)
            assert len(lanes) == c
            m[s, lanes] = True
        out[name] = m.reshape(-1)
    m = np.ones((len(HOLES), SLICE), dtype=bool)
    m[np.arange(len(HOLES)), HOLES] = False
    out["holes"] = m.reshape(-1)
    out["single"] = np.eye(SLICE, dtype=bool).reshape(-1)
    for tail in (1, 63):
        m = np.zeros(2 * SLICE + tail, dtype=bool)
        m[5:2 * SLICE:7] = True
        m[-1] = True
        out[f"last{tail}"] = m
    return {name: pooled(m, 100 + k) for k, (name, m) in enumerate(out.items())}


# ----------------------------------------------------------------------------- cap cases ---
CAP_SLICE_COUNTS = [64, 0, 17, 64, 5]
CAP_IN_FULL_SLICE = [15, 16, 17, 31, 32, 33, 48, 63]


def cap_case() -> Case:
    return pooled(mask_of(CAP_SLICE_COUNTS, SLICE * len(CAP_SLICE_COUNTS), 31), 31)


def caps() -> list:
    """Every slice's base, base + 1 and base + count; the round edges inside the first (full)
    slice; 0 and count + GUARD."""
    base = np.concatenate([[0], np.cumsum(CAP_SLICE_COUNTS)])
    c = set(CAP_IN_FULL_SLICE) | {0, int(base[-1]) + GUARD}
    for s, cnt in enumerate(CAP_SLICE_COUNTS):
        c |= {int(base[s]), int(base[s]) + 1, int(base[s]) + cnt}
    return sorted(c)


# -------------------------------------------------------------------------- length cases ---
LENGTHS = list(range(65)) + [65, 1514, 65535]


def length_case() -> Case:
    """Four frames of every length of LENGTHS, each at a pool line of its own, four in five of
    them resets.  dev_pool: every line's bytes from len to 64 set to 0xFF."""
    n = 4 * len(LENGTHS)
    lens = np.array([LENGTHS[i % len(LENGTHS)] for i in range(n)], dtype=np.uint16)
    pool = np.random.default_rng(64).integers(0, 255, n * 64, dtype=np.uint8)   # no 0xFF of its own
    poisoned = pool.reshape(n, 64).copy()
    poisoned[np.arange(64)[None, :] >= lens.astype(np.int64)[:, None]] = 0xFF
    return Case(pool, np.arange(n), lens, np.arange(n) % 5 != 3, 64, dev_pool=poisoned.reshape(-1))


# ---------------------------------------------------------------------- checksum corners ---
def base_offender() -> bytes:
    """A 64-byte line put together field by field: 172.16.5.9:40001 -> 192.168.78.2:9999, ACK."""
    eth = bytes([0x02, 0, 0xC0, 0xA8, 0x4E, 0x02]) + bytes([0x02, 0x11, 0x22, 0x33, 0x44, 0x55]) + b"\x08\x00"
    ip = struct.pack("!BBHHHBBH", 0x45, 0, 40, 0x1234, 0x4000, 64, 6, 0) + bytes([172, 16, 5, 9]) + bytes([192, 168, 78, 2])
    tcp = struct.pack("!HHIIBBHHH", 40001, 9999, 0x01020304, 0xA1B2C3D4, 0x50, 0x10, 0xFFFF, 0, 0)
    return eth + ip + tcp + bytes(10)


def ip_words(line) -> tuple:
    """The ten big-endian words of a reset's IPv4 header."""
    return struct.unpack("!10H", bytes(line[14:34]))


def tcp_words(line) -> tuple:
    """The big-endian words of a reset's pseudo header and TCP header."""
    return struct.unpack("!16H", bytes(line[26:34]) + b"\x00\x06\x00\x14" + bytes(line[34:54]))


def swapped(words) -> list:
    """The same bytes read as little-endian words, the way the kernel adds them."""
    return [((w & 0xFF) << 8) | (w >> 8) for w in words]


def _solve(f: bytearray, at: int, words, ip_id: int, kind: str):
    """Sets the offender's 16-bit field at `at`, taken as zero before, so that the reset's sum
    over words(..) is a multiple of 0xFFFF (kind "zero"), or, read as little-endian words, has
    a low half of 0xFFFF under a high half that is not 0 (kind "carry")."""
    f[at:at + 2] = b"\0\0"
    w = words(ref.reset_unsummed(bytes(f), ip_id, MAC))
    if kind == "zero":
        s = sum(w)
        f[at:at + 2] = ((0xFFFF - s % 0xFFFF) % 0xFFFF).to_bytes(2, "big")
    else:
        s = sum(swapped(w))
        assert s >> 16
        f[at:at + 2] = (0xFFFF - (s & 0xFFFF)).to_bytes(2, "little")


def corner_offender(kind: str, ip_id: int) -> bytes:
    """The 64-byte offender line of a checksum corner, for the packet id its reset will carry.
      ip     the reset's header sum folds to 0xFFFF, its checksum is 0x0000: the low half of the
             offender's source address (the reset's dst_addr, the header's last word) makes the
             big-endian words add up to a multiple of 0xFFFF
      tcp    the same for the TCP sum, through the low half of the offender's recv_ack (the
             reset's sent_seq), which the header sum does not see
      both   both at once
      carry  the first fold of both sums, added as the kernel adds them, leaves a carry: a low
             half of 0xFFFF under a high half that is not 0, so one fold gives 0x10000 or more
      ones   every byte 0xFF; meant for packet id 0xFFFF
      zero   every byte 0"""
    if kind == "ones":
        return b"\xff" * 64
    if kind == "zero":
        return bytes(64)
    assert kind in ("ip", "tcp", "both", "carry")
    f = bytearray(base_offender())
    if kind == "carry":
        f[30:34] = b"\xff" * 4      # the reset's src_addr: two words that put both sums past 16 bits
    how = "carry" if kind == "carry" else "zero"
    if kind != "tcp":
        _solve(f, 28, ip_words, ip_id, how)
    if kind != "ip":
        _solve(f, 44, tcp_words, ip_id, how)
    return bytes(f)


CORNER_KINDS = ["ip", "tcp", "both", "carry", "ones", "zero"]
CORNER_SLICE_COUNTS = [64, 17]
# the first reset of a slice, the last of a 16-reset round and the first of the next, the last
# reset of a full slice, the first and the last of a partial one
CORNER_RANKS = [0, 15, 16, 63, 64, 80]


def corner_case(rotation: int) -> Case:
    """Two slices of 64 and 17 resets; the reset of rank CORNER_RANKS[t] answers the corner line of
    kind CORNER_KINDS[(t + rotation) % 6], built for the packet id that rank carries.  ip_id0 is
    chosen so that the all-0xFF line's reset carries 0xFFFF.  named: kind -> reset number."""
    c = pooled(mask_of(CORNER_SLICE_COUNTS, SLICE * len(CORNER_SLICE_COUNTS), 55), 55 + rotation,
               lens=np.full(SLICE * len(CORNER_SLICE_COUNTS), 64, np.uint16))
    named = {CORNER_KINDS[(t + rotation) % len(CORNER_KINDS)]: k for t, k in enumerate(CORNER_RANKS)}
    ip_id0 = (0xFFFF - named["ones"]) & 0xFFFF
    frames = np.nonzero(c.mask)[0]
    lines = [np.frombuffer(corner_offender(kind, (ip_id0 + k) & 0xFFFF), np.uint8) for kind, k in named.items()]
    off = c.off.copy()
    for j, k in enumerate(named.values()):
        off[frames[k]] = POOL_LINES + j
    return Case(np.concatenate([c.pool] + lines), off, c.lens, c.mask, c.seed, ip_id0=ip_id0, named=named)
