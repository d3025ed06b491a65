"""Deterministic receive-checksum cases: the end of the TCP span walked across every chunk and
lane boundary of every size class (rxg_rx_frames.h: fields_small, frame_round_compute's eight
streaming classes, frame_fields<64, 2, JUMBO>), one-bit flips at every byte of a frame, the
largest sums and the 0x0000 / 0xFFFF corner.

Every builder is seeded and returns (rows, frames) ready for pktgen.pack_arena /
pktgen.table_arrays.  Frames come from pktgen.frame; where total_length is overwritten both
checksums are rewritten with pktgen.ip_checksum_of / pktgen.tcp_checksum_of, the pure-Python
restatement (not the oracle).  A frame tells its own cell: describe(frame).
"""
from __future__ import annotations

import functools
import random
import struct

import pktgen

# (lowest, highest data_len, lanes per frame) of the receive kernel's size classes, by
# length; a round of a class holds 64 / LPF frames.  Jumbo stops at 4200 here: the 2048
# bytes held in registers and three streamed steps of 1024.
CLASSES = [(0, 64, 1), (65, 128, 2), (129, 256, 4), (257, 512, 8), (513, 576, 8), (577, 768, 8),
           (769, 1024, 16), (1025, 1536, 16), (1537, 2048, 32), (2049, 4200, 64)]
JUMBO = len(CLASSES) - 1
MIN_LEN = 54  # whole Ethernet + IPv4 + TCP headers
FLIP_LENGTHS = [64, 128, 256, 512, 576, 768, 1024, 1536, 2048, 4133]


def class_of(length: int) -> int:
    """Index into CLASSES of a frame length (jumbo: everything over 2048)."""
    for k, (_lo, hi, _lpf) in enumerate(CLASSES[:-1]):
        if length <= hi:
            return k
    return JUMBO


def total_length_of(f: bytes) -> int:
    return struct.unpack(">H", f[16:18])[0]


def tcp_end_of(f: bytes) -> int:
    """End of the TCP span: 14 + total_length, at least 34, clamped by the frame's end."""
    return min(len(f), max(34, 14 + total_length_of(f)))


def describe(f: bytes) -> str:
    lo, hi, _ = CLASSES[class_of(len(f))]
    return f"class {lo}-{hi}, L {len(f)}, total_length {total_length_of(f)}, tcp_end {tcp_end_of(f)}"


def rewrite_checksums(b: bytearray) -> bytes:
    """Both stored checksums of a frame of at least 54 bytes, from the Python restatement."""
    b[24:26] = b"\0\0"
    b[24:26] = struct.pack(">H", pktgen.ip_checksum_of(bytes(b)))
    b[50:52] = b"\0\0"
    b[50:52] = struct.pack(">H", pktgen.tcp_checksum_of(bytes(b)))
    return bytes(b)


def with_total_length(f: bytes, tl: int) -> bytes:
    b = bytearray(f)
    b[16:18] = struct.pack(">H", tl)
    return rewrite_checksums(b)


def zeroed_fields(f: bytes) -> bytes:
    """The frame as tx checksum generate receives it: both checksum fields zero."""
    return f[:24] + b"\0\0" + f[26:50] + b"\0\0" + f[52:]


def grid_lengths(k: int) -> list[int]:
    """Class minimum, minimum + 1, maximum - 1, maximum, and every multiple of 16 in the class
    with the multiple +- 1; lengths of at least 54 that belong to the class."""
    lo, hi, _ = CLASSES[k]
    want = {lo, lo + 1, hi - 1, hi}
    for m in range((lo + 15) // 16 * 16, hi + 1, 16):
        want |= {m - 1, m, m + 1}
    return sorted(x for x in want if max(lo, MIN_LEN) <= x <= hi)


def grid_total_lengths(length: int) -> list[int]:
    """E = 14 + total_length below 34, at 34, on both sides of 48 and of the checksum field, one
    chunk short of the frame's end, just short of it, at it and past it, and the
    (total_length - 20) & 0xFFFF wrap."""
    d = length - 14
    want = {0, 1, 19, 20, 21, 33, 34, 35, 39, 40, 41, d - 17, d - 16, d - 15, d - 1, d, d + 1, d + 16, 65535}
    return sorted(x for x in want if 0 <= x <= 65535)


def _table(rng):
    rows, flows, _special = pktgen.parity_table(rng, 64)
    return rows, flows


def _base_frame(rng, flows, length: int) -> bytes:
    src, sport, dport = rng.choice(flows)
    f = pktgen.frame(src_ip=src, sport=sport, dport=dport, seq=rng.getrandbits(32), ack=rng.getrandbits(32),
                     flags=rng.choice([0x10, 0x18, 0x02, 0x11]), ip_id=rng.getrandbits(16),
                     payload=rng.randbytes(length - MIN_LEN))
    assert len(f) == length
    return f


@functools.lru_cache(maxsize=None)
def _span_grid():
    rng = random.Random(0x5BA9)
    rows, flows = _table(rng)
    frames = []
    for k in range(len(CLASSES)):
        for length in grid_lengths(k):
            base = _base_frame(rng, flows, length)
            assert class_of(length) == k
            for tl in grid_total_lengths(length):
                frames.append(with_total_length(base, tl))
    return rows, tuple(frames)


def span_grid():
    """The grid as generated: class after class, length after length, the total_lengths of one
    length together, so whole rounds are uniformly slow-span (tcp_end < len) or uniformly fast."""
    rows, frames = _span_grid()
    return rows, list(frames)


def rounds_of(frames):
    """The rounds the kernel forms: per 64-frame slice, each class's frames compacted in order
    and taken 64 / LPF at a time.  Yields (class index, [frames of the round])."""
    for s in range(0, len(frames), 64):
        by_class: dict[int, list[bytes]] = {}
        for f in frames[s:s + 64]:
            by_class.setdefault(class_of(len(f)), []).append(f)
        for k, fs in by_class.items():
            fpw = 64 // CLASSES[k][2]
            for r in range(0, len(fs), fpw):
                yield k, fs[r:r + fpw]


def mixed_round_classes(frames) -> set[int]:
    """Classes with at least one full round of consecutive frames that holds both kinds: a frame
    whose span ends before its end, and one whose span is the whole frame.  (Class 0 has 33 grid
    frames, fewer than its round of 64: its one partly filled round counts.)"""
    got = set()
    for k, fs in rounds_of(frames):
        fpw = 64 // CLASSES[k][2]
        kinds = {tcp_end_of(f) < len(f) for f in fs}
        if (len(fs) == fpw or k == 0) and len(kinds) == 2:
            got.add(k)
    return got


@functools.lru_cache(maxsize=None)
def _span_grid_interleaved():
    rows, frames = _span_grid()
    rng = random.Random(0x1E4F)
    out = []
    for k in range(len(CLASSES)):
        fs = [f for f in frames if class_of(len(f)) == k]
        rng.shuffle(fs)
        out.extend(fs)
    # a condition on the input: the per-frame select after the wave-uniform slow-span branch
    # needs rounds whose frames disagree (a jumbo round is one frame: nothing to mix)
    missing = set(range(JUMBO)) - mixed_round_classes(out)
    assert not missing, f"no mixed round in classes {sorted(missing)}"
    return rows, tuple(out)


def span_grid_interleaved():
    """The same frames shuffled within each class, so the frames of one round alternate between
    tcp_end < len and tcp_end == len."""
    rows, frames = _span_grid_interleaved()
    return rows, list(frames)


def class_slices(frames):
    """{class index: the frames of that class, in order}."""
    out: dict[int, list[bytes]] = {}
    for f in frames:
        out.setdefault(class_of(len(f)), []).append(f)
    return out


def small_layouts(nslices: int = 64):
    """The class-0 part of the grid twice, each as `nslices` slices of 64 frames: whole slices of
    small frames (the all-small pipeline), and every slice holding at least one longer frame
    (run_class<0, 1, 4> with the LDS transpose).  Returns (rows, all_small, mixed)."""
    rows, frames = _span_grid()
    small = [f for f in frames if len(f) <= 64]
    longer = [next(f for f in frames if class_of(len(f)) == k and tcp_end_of(f) == len(f))
              for k in range(1, len(CLASSES))]
    n = 64 * nslices
    assert n >= 4 * len(small)
    all_small = [small[i % len(small)] for i in range(n)]
    rng = random.Random(0x51AB)
    mixed = list(all_small)
    for s in range(nslices):
        for _ in range(1 + s % 3):
            mixed[64 * s + rng.randrange(64)] = longer[rng.randrange(len(longer))]
    for s in range(nslices):
        assert all(len(f) <= 64 for f in all_small[64 * s:64 * s + 64])
        assert any(len(f) > 64 for f in mixed[64 * s:64 * s + 64])
    assert set(small) <= set(all_small) and set(small) <= set(mixed)
    return rows, all_small, mixed


# ------------------------------------------------------------------------- flip set ---

@functools.lru_cache(maxsize=None)
def _flip_set(shorten: int):
    rng = random.Random(0xF11B + shorten)
    rows, flows = _table(rng)
    frames, base_of = [], []
    for length in FLIP_LENGTHS:
        base = _base_frame(rng, flows, length)
        if shorten:
            base = with_total_length(base, total_length_of(base) - shorten)
        b0 = len(frames)
        frames.append(base)
        base_of.append(b0)
        for p in range(14, length):
            g = bytearray(base)
            g[p] ^= 1
            frames.append(bytes(g))
            base_of.append(b0)
    return rows, tuple(frames), tuple(base_of)


def flip_set(shorten: int = 0):
    """Per class one valid frame at the class maximum (4133 for jumbo), then a copy for every
    byte position p in [14, L) with bit 0 of byte p flipped; shorten: total_length less by that
    much (checksums rewritten), so the span ends before the frame does.  Returns (rows, frames,
    base_of): base_of[i] is the index of frame i's unflipped baseline (its own for a baseline;
    the flipped byte of frame i is 14 + i - base_of[i] - 1)."""
    rows, frames, base_of = _flip_set(shorten)
    return rows, list(frames), list(base_of)


def check_flip_rules(frames, base_of, c, shorten):
    """The three rules on records c (rxg_rec16 fields); the host test applies them to the
    oracle's records, the GPU test to the kernel's."""
    n_ip = n_tcp = n_past = want_past = 0
    for i, f in enumerate(frames):
        b = base_of[i]
        if b == i:  # a baseline: valid
            te = tcp_end_of(f)
            assert len(f) in FLIP_LENGTHS and te == max(34, len(f) - shorten)
            # (64 bytes less 40: the span ends at 34, before the checksum field)
            assert c["ip_cksum"][i] == 0 and (c["tcp_cksum"][i] == 0) == (te >= 52), describe(f)
            want_past += len(f) - te
            continue
        p = 14 + i - b - 1
        base = frames[b]
        assert f[p] == base[p] ^ 1 and f[:p] == base[:p] and f[p + 1:] == base[p + 1:]
        te = tcp_end_of(base)
        where = f"{describe(base)}, flipped byte {p} (lane {p // 16 % CLASSES[class_of(len(f))][2]})"
        if 14 <= p <= 33:
            n_ip += 1
            assert c["ip_cksum"][i] != 0, where
        if 26 <= p < te:
            n_tcp += 1
            assert c["tcp_cksum"][i] != c["tcp_cksum"][b] and (c["tcp_cksum"][i] != 0 or te < 52), where
        if p >= te:
            n_past += 1
            assert c["ip_cksum"][i] == c["ip_cksum"][b] == 0 and c["tcp_cksum"][i] == c["tcp_cksum"][b], where
    assert n_ip == 20 * len(FLIP_LENGTHS) and n_tcp > 10000
    assert n_past == want_past and (n_past > 0) == (shorten > 0)


# ---------------------------------------------------------------------- extreme set ---

def _with_zero_tcp_checksum(f: bytes) -> bytes:
    """The frame with one payload word chosen so the stored TCP checksum is 0x0000: with the
    word zero the checksum is the complement of the folded sum S of the rest, and S + ~S =
    0xFFFF, so the word wanted is that checksum's two bytes."""
    w = (len(f) - 3) & ~1  # an even offset, both bytes inside the frame and the span
    assert w >= 54 and tcp_end_of(f) == len(f)
    b = bytearray(f)
    b[w:w + 2] = b"\0\0"
    b = bytearray(rewrite_checksums(b))
    b[w:w + 2] = b[50:52]
    out = rewrite_checksums(b)
    assert out[50:52] == b"\0\0", describe(f)
    return out


def _with_zero_ip_checksum(f: bytes) -> bytes:
    """The same with ip_id as the free word and the IPv4 header checksum."""
    b = bytearray(f)
    b[18:20] = b"\0\0"
    b = bytearray(rewrite_checksums(b))
    b[18:20] = b[24:26]
    out = rewrite_checksums(b)
    assert out[24:26] == b"\0\0", describe(f)
    return out


@functools.lru_cache(maxsize=None)
def _extreme_set():
    rng = random.Random(0xE87E)
    rows, flows = _table(rng)
    frames, kinds = [], []
    # the largest and the smallest sums: bytes from 34 on all 0xFF / all zero.  As built the TCP
    # checksum field is part of the fill (the frame does not verify: the oracle says what it
    # gives); a second copy has the field rewritten and verifies.  total_length 65535 is clamped
    # by the frame's end; with 65521 the span ends at byte 65535, the longest frame's last.
    for length in (9018, 65535):
        for fill in (0xFF, 0x00):
            for tl in (65535, 65521):
                src, sport, dport = flows[(length + tl) % len(flows)]
                head = pktgen.frame(src_ip=src, sport=sport, dport=dport)[:34]
                b = bytearray(head + bytes([fill]) * (length - 34))
                b[16:18] = struct.pack(">H", tl)
                b[24:26] = b"\0\0"
                b[24:26] = struct.pack(">H", pktgen.ip_checksum_of(bytes(b)))
                frames.append(bytes(b))
                kinds.append("fill")
                frames.append(rewrite_checksums(b))
                kinds.append("fill_valid")
    # stored checksums of 0x0000, and 0xFFFF in their place: the two representations of one
    # one's-complement value, so both verify
    for k, (lo, hi, _lpf) in enumerate(CLASSES):
        length = {0: 64, JUMBO: 4133}.get(k, (lo + hi) // 2 | 1)
        base = _base_frame(rng, flows, length)
        z = _with_zero_tcp_checksum(base)
        frames += [z, z[:50] + b"\xff\xff" + z[52:]]
        kinds += ["tcp_0000", "tcp_ffff"]
        z = _with_zero_ip_checksum(base)
        frames += [z, z[:24] + b"\xff\xff" + z[26:]]
        kinds += ["ip_0000", "ip_ffff"]
    return rows, tuple(frames), tuple(kinds)


def extreme_set():
    """Returns (rows, frames, kinds); kinds[i] in {"fill", "fill_valid", "tcp_0000", "tcp_ffff",
    "ip_0000", "ip_ffff"}: every kind but "fill" must verify (both checksums zero)."""
    rows, frames, kinds = _extreme_set()
    return rows, list(frames), list(kinds)
