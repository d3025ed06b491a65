"""Deterministic tables, queries and slice layouts for the device flow lookup
(dpdk-tcpipstack_amd/csrc/rxg_rx_classify.h): the home-bucket fetch in its three forms, the
overflow walks over tuples and ARP addresses, and the per-lane flow cache.  No GPU, no
randomness beyond fixed seeds.

The hashes of rxg_common.h are restated here so that a table can be built with chosen home
buckets: Finder walks a fixed range (sources 10.x.y.z, source ports from 1024) and hands out the
first tuples whose hash lands where it is asked to.  Where a key ends up after TcbMirror::rebuild
depends on the iteration order of an unordered map, so a table never relies on it: the number of
keys per bucket does not depend on the order (linear probing), which fixes the walk of every
*missing* tuple; a *found* key that has to walk is upserted after the load (Table.ops), when its
home bucket is known to be full.  tests/lookup_check.cpp reports where the host mirror really put
things, and test_lookup_cases_host.py holds every label below against it.
"""
from __future__ import annotations

import functools
import random
import struct
from collections import namedtuple

import pktgen
from pktgen import ESTABLISHED, LISTENING, ip4, raw_of_host

M32 = 0xFFFFFFFF
DST = ip4(192, 168, 78, 2)
DST_RAW = raw_of_host(DST)
SYN, ACK = 0x02, 0x10
WALKER_LANES = (0, 1, 31, 32, 33, 62, 63)
PARTIAL_SIZES = (1, 3, 4, 5, 63)
FORMS = ("small", "class", "alt")


# ------------------------------------------------------------------------------ hashes ---

def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def tuple_hash(ports, dst_raw, src_host):
    """rxg_common.h tuple_hash."""
    h = 0x9E3779B9 ^ ((ports * 0xCC9E2D51) & M32)
    h = (_rotl(h, 13) * 5 + 0xE6546B64) & M32
    h ^= (_rotl((dst_raw * 0xCC9E2D51) & M32, 15) * 0x1B873593) & M32
    h = (_rotl(h, 13) * 5 + 0xE6546B64) & M32
    h ^= (_rotl((src_host * 0xCC9E2D51) & M32, 15) * 0x1B873593) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def arp_hash(ip):
    """rxg_common.h arp_hash."""
    h = (ip ^ 0x41525000) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def tcb_nb(nkeys):
    """TcbMirror::rebuild: the smallest power of two with 2 * nb >= keys."""
    nb = 1
    while 2 * nb < nkeys:
        nb <<= 1
    return nb


def arp_nb(naddr):
    """ArpMirror::rebuild: the smallest power of two >= 4 with 2 * nb >= addresses."""
    nb = 4
    while 2 * nb < naddr:
        nb <<= 1
    return nb


# A query: the tuple a frame carries (dst: the host-order address put on the wire), what findtcb
# makes of it (kind: found / listen / listen_null / nopcb) and whether the lookup leaves the home
# bucket (walk: True, False, or None where that depends on the rebuild's order).
Q = namedtuple("Q", "label src sport dport dst kind walk")


def key_of(q):
    """The three words pass 1 compares (tcp_tcb.c:152-155)."""
    return ((q.dport << 16) | q.sport, raw_of_host(q.dst), q.src)


def home_of(q, mask):
    return tuple_hash(*key_of(q)) & mask


class Finder:
    """The first tuples of the walk 10.x.y.z / sport 1024.. with a wanted home bucket; no tuple is
    handed out twice."""

    def __init__(self, mask, start=1):
        self.mask, self.i = mask, start

    def take(self, home, k, dport=80, dst=DST):
        out = []
        while len(out) < k:
            i = self.i
            self.i += 1
            src, sport = ip4(10, (i >> 16) & 255, (i >> 8) & 255, i & 255), 1024 + (i >> 24)
            if tuple_hash((dport << 16) | sport, raw_of_host(dst), src) & self.mask == home:
                out.append((src, sport, dport))
        return out


def arp_addresses(mask, home, k, start=1, avoid=()):
    """The first k addresses 10.200.y.z from `start` whose arp_hash lands in bucket `home`."""
    out, i = [], start
    while len(out) < k:
        ip = ip4(10, 200, (i >> 8) & 255, i & 255)
        if arp_hash(ip) & mask == home and ip not in avoid:
            out.append(ip)
        i += 1
    return out


def occupancy(homes, nb):
    """Keys per bucket after inserting keys with these home buckets (any order gives the same)."""
    occ = [0] * nb
    for h in homes:
        while occ[h] == 4:
            h = (h + 1) % nb
        occ[h] += 1
    return occ


def miss_probes(occ, home):
    """Buckets a missing key with this home reads: up to the first bucket with a free slot."""
    n, nb = 1, len(occ)
    while occ[home] == 4 and n < nb:
        home, n = (home + 1) % nb, n + 1
    return n


# ------------------------------------------------------------------------------ tables ---

class Table:
    """rows: tcbs[] as loaded (pktgen.table_arrays).  ops: writes made after the load has been
    synchronised, in order: ("upsert", idx, row) / ("remove", idx).  final_rows: tcbs[] after them
    (what the oracle classifies against).  queries: list of Q.  nb: the bucket count stated."""

    def __init__(self, name, rows, queries, nb, ops=()):
        self.name, self.rows, self.queries, self.nb, self.ops = name, rows, queries, nb, list(ops)
        self.final_rows = apply_ops(rows, self.ops)
        assert len({q.label for q in queries}) == len(queries), name
        # a missing tuple's walk follows from the keys per bucket alone
        keys = distinct_keys(self.final_rows)
        self.occ = occupancy([tuple_hash(*k) & (nb - 1) for k in sorted(keys)], nb)
        self.queries = [q if q.kind in ("found", None) or key_of(q) in keys else
                        q._replace(walk=miss_probes(self.occ, home_of(q, nb - 1)) >= 2) for q in queries]

    def q(self, label):
        return next(x for x in self.queries if x.label == label)

    @property
    def walkers(self):
        return [q for q in self.queries if q.walk is True]

    @property
    def still(self):
        return [q for q in self.queries if q.walk is False]

    def loaded_keys(self):
        return distinct_keys(self.rows)


def apply_ops(rows, ops):
    rows = list(rows)
    for op in ops:
        if op[0] == "remove":
            rows[op[1]] = None
        else:
            rows.extend([None] * (op[1] + 1 - len(rows)))
            rows[op[1]] = op[2]
    return rows


def distinct_keys(rows):
    keys = set()
    for r in rows:
        if r is not None and 0 <= r[0] <= 65535 and 0 <= r[1] <= 65535:
            keys.add(((r[0] << 16) | r[1], r[2] & M32, r[3] & M32))
    return keys


def _row(t, state, dst_raw=DST_RAW):
    src, sport, dport = t
    return (dport, sport, dst_raw, src, state)


def _q(label, t, kind, walk, dst=DST):
    return Q(label, t[0], t[1], t[2], dst, kind, walk)


_STATES = [2, 3, 4, 5, 6, 0]
ZERO_Q = Q("zero", 0, 0, 0, 0, None, None)


@functools.lru_cache(maxsize=None)
def tiny_wrap():
    """nb = 2, four keys all with home 1: bucket 1 is full, bucket 0 empty."""
    f = Finder(1)
    k = f.take(1, 4)
    rows = [_row(k[0], LISTENING)] + [_row(t, _STATES[i]) for i, t in enumerate(k[1:])]
    qs = [_q(f"key{i}", t, "found", False) for i, t in enumerate(k)]
    qs += [_q("miss1_listen", f.take(1, 1)[0], "listen", True),       # walks 1 -> 0 across the end
           _q("miss1_nopcb", f.take(1, 1, dport=9999)[0], "nopcb", True),
           _q("miss0_listen", f.take(0, 1)[0], "listen", False),
           _q("miss0_nopcb", f.take(0, 1, dport=9999)[0], "nopcb", False)]
    return Table("tiny_wrap", rows, qs, 2)


def _cluster16(removed):
    """nb = 16.  Loaded: 14 keys with home 14 (buckets 14, 15, 0 and half of 1, whatever the
    order) and 12 with homes 4-11, two of them listeners (:80, and :8080 behind a removed slot).
    Upserted after the load, so their places are known: two keys with home 15 (bucket 15 and 0
    full: both land in 1, two buckets on), two with home 0 (0 and 1 full: in 2), one with home 1
    (in 2) and one with home 2 (fills 2).  Buckets 14, 15, 0, 1, 2 are then full and 3 is empty: a
    missing tuple with home 14 / 15 / 0 / 1 / 2 reads 6 / 5 / 4 / 3 / 2 buckets."""
    f = Finder(15)
    rng = random.Random(16)
    h14 = f.take(14, 14)
    rest = [t for h, n in ((4, 2), (6, 2), (8, 2), (9, 1), (10, 2), (11, 1)) for t in f.take(h, n)]
    l80, l8080 = f.take(5, 1)[0], f.take(7, 1, dport=8080)[0]   # the listeners' own keys: 12 in 4-11
    plain = [(t, f"h14_{i}") for i, t in enumerate(h14)] + [(t, f"rest{i}") for i, t in enumerate(rest)]
    rng.shuffle(plain)
    half = len(plain) // 2
    order = [(l80, "l80")] + plain[:half] + [None] + [(l8080, "l8080")] + plain[half:]
    rows, qs, idx_of = [], [], {}
    for i, e in enumerate(order):
        if e is None:
            rows.append(None)
            continue
        t, label = e
        idx_of[label] = i
        st = LISTENING if label.startswith("l8") else _STATES[(i * 5 + 1) % 6]
        rows.append(_row(t, st))
        qs.append(_q(label, t, "found", None if label.startswith("h14") else False))
    late = [("h15a", f.take(15, 1)[0], True), ("h15b", f.take(15, 1)[0], True), ("h0a", f.take(0, 1)[0], True),
            ("h0b", f.take(0, 1)[0], True), ("h1", f.take(1, 1)[0], True), ("h2", f.take(2, 1)[0], False)]
    ops = []
    for j, (label, t, walk) in enumerate(late):
        idx_of[label] = len(rows) + j
        ops.append(("upsert", len(rows) + j, _row(t, _STATES[j % 6])))
        qs.append(_q(label, t, "found", walk))
    for home, dport, kind in [(14, 80, "listen"), (15, 9999, "nopcb"), (0, 8080, "listen_null"), (0, 80, "listen"),
                              (1, 9999, "nopcb"), (1, 80, "listen"), (2, 80, "listen"), (2, 8080, "listen_null"),
                              (6, 80, "listen"), (6, 9999, "nopcb"), (9, 8080, "listen_null")]:
        qs.append(_q(f"miss{home}_{kind}", f.take(home, 1, dport=dport)[0], kind, home not in (6, 9)))
    name = "cluster16"
    if removed:
        # Seven of the fourteen home-14 keys go (at most six of them sit past the table's end, and
        # keys only ever move towards home: one removal hits bucket 14 or 15, and the backward
        # shift then pulls a key across the end), three come back in another state.
        name = "cluster16_removed"
        gone = [idx_of[f"h14_{i}"] for i in (0, 2, 3, 5, 7, 8, 11)]
        ops += [("remove", i) for i in gone]
        ops += [("upsert", i, rows[i][:4] + (ESTABLISHED,)) for i in gone[:3]]
        dead = {f"h14_{i}" for i in (5, 7, 8, 11)}
        cluster = {f"h14_{i}" for i in range(14)} | {"h15a", "h15b", "h0a", "h0b", "h1", "h2"}
        qs = [q._replace(kind="listen") if q.label in dead else q._replace(walk=None) if q.label in cluster else q
              for q in qs]
    t = Table(name, rows, qs, 16, ops)
    t.idx_of = idx_of
    t.setup_ops = 6  # the upserts that belong to the table itself
    return t


@functools.lru_cache(maxsize=None)
def cluster16():
    return _cluster16(False)


@functools.lru_cache(maxsize=None)
def cluster16_removed():
    return _cluster16(True)


@functools.lru_cache(maxsize=None)
def zero_tuple(live, full):
    """nb = 8 and the all-zero tuple, whose key words equal a free slot's.  full: thirteen keys
    share its home bucket (14 when it is absent), so the query reads four buckets and ends in one
    with free slots; live and full, it is upserted after the load and sits three buckets on."""
    f = Finder(7)
    hz = tuple_hash(0, 0, 0) & 7
    zero_row = (0, 0, 0, 0, ESTABLISHED)
    if full:
        cl = f.take(hz, 13 if live else 14)
        other = f.take((hz + 5) & 7, 2, dport=0)
        rows = [_row(other[0], LISTENING)] + [_row(t, _STATES[i % 6]) for i, t in enumerate(cl)] + [_row(other[1], 3)]
        ops = [("upsert", len(rows), zero_row)] if live else []
        qs = [_q("listen0", other[0], "found", False), _q("other", other[1], "found", False)]
        qs += [_q(f"hz{i}", t, "found", None) for i, t in enumerate(cl)]
        qs += [_q("miss_hz", f.take(hz, 1)[0], "nopcb", True),
               _q("miss_free", f.take((hz + 6) & 7, 1)[0], "nopcb", False)]
        zq = ZERO_Q._replace(kind="found" if live else "listen", walk=True)
    else:
        keys = f.take(hz, 1) + [t for h in range(8) if h != hz for t in f.take(h, 1)] + f.take((hz + 1) & 7, 1)
        rows = [_row(t, _STATES[i % 6]) for i, t in enumerate(keys)]
        if live:
            rows.insert(4, zero_row)
        ops = []
        qs = [_q(f"key{i}", t, "found", False) for i, t in enumerate(keys)]
        qs.append(_q("miss_hz", f.take(hz, 1)[0], "nopcb", False))
        zq = ZERO_Q._replace(kind="found" if live else "nopcb", walk=False)
    t = Table(f"zero_{'live' if live else 'absent'}_{'full' if full else 'free'}", rows, qs + [zq], 8, ops)
    t.setup_ops = len(ops)
    return t


ZERO_FORMS = [(True, False), (False, False), (True, True), (False, True)]


@functools.lru_cache(maxsize=None)
def duplicates():
    """findtcb's quirks: a tuple held by three indices whose lowest is removed after the load (the
    next lowest answers), int ports outside 0..65535, a host-order ipv4_dst, a LISTENING slot with
    a full tuple (pktgen.parity_table's special cases), among eight plain keys; nb = 8."""
    f = Finder(7, start=5000)
    dup = f.take(3, 1)[0]
    plain = [f.take(h, 1)[0] for h in range(8)]
    lt, bad1, bad2, hd = (ip4(10, 9, 9, 9), 4242, 443), (ip4(10, 8, 8, 8), 5000, -1), (ip4(10, 8, 8, 9), 5001, 70000), \
        (ip4(10, 7, 7, 7), 6000, 80)
    rows = [(80, 0, DST_RAW, 0, LISTENING), _row(dup, 3), _row(plain[0], 4), _row(dup, 5), _row(plain[1], 2),
            _row(dup, 6), _row(lt, LISTENING), _row(bad1, 4), _row(bad2, 4), _row(hd, 4, dst_raw=DST)]
    rows += [_row(t, _STATES[i % 6]) for i, t in enumerate(plain[2:])]
    qs = [_q("dup", dup, "found", None), _q("listen_tuple", lt, "found", None),
          _q("badport_m1", (bad1[0], bad1[1], 65535), "nopcb", None),
          _q("badport_70000", (bad2[0], bad2[1], 70000 & 0xFFFF), "nopcb", None),
          _q("hostdst", hd, "listen", None), _q("listener_own", (0, 0, 80), "found", None),
          _q("miss443", (ip4(10, 9, 9, 8), 4242, 443), "listen_null", None)]
    qs += [_q(f"plain{i}", t, "found", None) for i, t in enumerate(plain)]
    t = Table("duplicates", rows, qs, 8, [("remove", 1)])
    t.setup_ops = 1
    return t


@functools.lru_cache(maxsize=None)
def rotation64():
    """nb = 32, 64 keys with distinct indices: 14 with home 30 (buckets 30, 31, 0 and half of 1),
    50 two to a bucket in 3-27."""
    f = Finder(31, start=9000)
    keys = f.take(30, 14) + [t for h in range(3, 28) for t in f.take(h, 2)]
    rng = random.Random(64)
    rng.shuffle(keys)
    rows = [_row(t, _STATES[(i * 5 + 2) % 6]) for i, t in enumerate(keys)]
    qs = [_q(f"key{i}", t, "found", None) for i, t in enumerate(keys)]
    return Table("rotation64", rows, qs, 32)


@functools.lru_cache(maxsize=None)
def cache_table():
    """nb = 64: sixteen base keys, each with the four keys that differ from it in bit 0 of sport,
    of dport (80 / 81), of src and of dst, under other indices; listeners on :80, :81 and, behind a
    removed slot, :8080."""
    f = Finder(63, start=20000)
    base = [f.take(h, 1)[0] for h in range(2, 34, 2)]
    rows = [(80, 0, DST_RAW, 0, LISTENING), (81, 0, DST_RAW, 0, LISTENING)]
    qs = []
    for j, (src, sport, dport) in enumerate(base):
        rows.append(_row((src, sport, dport), _STATES[j % 6]))
        rows.append(_row((src, sport ^ 1, dport), _STATES[(j + 1) % 6]))
        rows.append(_row((src, sport, dport ^ 1), _STATES[(j + 2) % 6]))
        rows.append(_row((src ^ 1, sport, dport), _STATES[(j + 3) % 6]))
        rows.append(_row((src, sport, dport), _STATES[(j + 4) % 6], dst_raw=raw_of_host(DST ^ 1)))
        qs.append(_q(f"base{j}", (src, sport, dport), "found", None))
    rows += [None, (8080, 0, DST_RAW, 0, LISTENING)]
    for j in range(16):
        qs.append(_q(f"miss80_{j}", (ip4(172, 16, 1, 2 * j), 3000 + 2 * j, 80), "listen", None))
        qs.append(_q(f"miss9998_{j}", (ip4(172, 16, 2, 2 * j), 3000 + 2 * j, 9998), "nopcb", None))
        qs.append(_q(f"miss8080_{j}", (ip4(172, 16, 3, 2 * j), 3000 + 2 * j, 8080), "listen_null", None))
    return Table("cache_table", rows, qs, 64)


def launched_tables():
    return [tiny_wrap(), cluster16(), cluster16_removed(), duplicates(), rotation64()] + \
        [zero_tuple(*z) for z in ZERO_FORMS]


# ------------------------------------------------------------------------------ frames ---

@functools.lru_cache(maxsize=None)
def _frame(src, dst, sport, dport, flags, plen):
    return pktgen.frame(src_ip=src, dst_ip=dst, sport=sport, dport=dport, flags=flags, seq=plen * 977 + 1,
                        ack=sport, payload=bytes((7 * i + plen) & 255 for i in range(plen)))


def plen_of(small, n):
    """Payload bytes of the n-th frame of a slice: 54-64 byte frames, or 65-128."""
    return (n * 7) % 11 if small else 11 + (n * 13) % 64


def q_frame(q, small, n, flags=ACK):
    return _frame(q.src, q.dst, q.sport, q.dport, flags, plen_of(small, n))


@functools.lru_cache(maxsize=None)
def other_frame(kind, small, n):
    """Frames that are no TCP segment: IPv4 / UDP, ARP, another ethertype."""
    pad = plen_of(small, n)
    if kind == "udp":
        return pktgen.frame(proto=17, src_ip=ip4(10, 3, 3, n & 255), payload=bytes(pad))
    if kind == "arp":
        body = struct.pack(">HHBBH", 1, 0x0800, 6, 4, 1 + (n & 1)) + bytes((n + i) & 255 for i in range(20))
        return b"\xff" * 6 + b"\x02\0\0\0\0\x07" + b"\x08\x06" + body + bytes(12 + pad)
    return bytes(12) + b"\x86\xdd" + bytes((n * 3 + i) & 255 for i in range(40 + pad))


def small_of(form, s):
    """Is slice s of a burst in this size form made of frames of at most 64 bytes?"""
    return form == "small" or (form == "alt" and s % 2 == 0)


# A slice is a list of up to 64 entries (Q, tcp flags) or ("other", kind) or ("raw", bytes_small,
# bytes_class); a burst is a list of slices of which only the last may be short.

def burst_frames(burst, form, small_fn=small_of):
    frames = []
    for s, sl in enumerate(burst):
        small = small_fn(form, s)
        for n, e in enumerate(sl):
            if e[0] == "other":
                frames.append(other_frame(e[1], small, n))
            elif e[0] == "raw":
                frames.append(e[1] if small else e[2])
            else:
                frames.append(q_frame(e[0], small, n, e[1]))
    return frames


def _flags(lane, s):
    return SYN if (lane + s) % 3 == 0 else ACK


def _still_slice(t, s, n=64):
    st = t.still
    return [(st[(lane + 3 * s) % len(st)], _flags(lane, s)) for lane in range(n)]


LANE_PATTERNS = [("all", range(64)), ("even", range(0, 64, 2)), ("odd", range(1, 64, 2)),
                 ("low", range(0, 32)), ("high", range(32, 64))]


def lane_walkers(t):
    """One burst of 12 slices over a table with walkers: a single walking lookup on lane 0, 1, 31,
    32, 33, 62, 63 among lookups that end in their home bucket, then every lane walking, the even
    lanes, the odd ones, lanes 0-31 and lanes 32-63.  The walkers of a slice differ in length and
    result as far as the table's do.  Returns (burst, [the walking lanes of each slice])."""
    w = t.walkers
    assert w and t.still, t.name
    burst, lanes = [], []
    for k, lane in enumerate(WALKER_LANES):
        sl = _still_slice(t, k)
        sl[lane] = (w[k % len(w)], _flags(lane, k))
        burst.append(sl)
        lanes.append({lane})
    for k, (_, ls) in enumerate(LANE_PATTERNS):
        s = len(WALKER_LANES) + k
        sl = _still_slice(t, s)
        for lane in ls:
            sl[lane] = (w[(lane + k) % len(w)], _flags(lane, s))
        burst.append(sl)
        lanes.append(set(ls))
    return burst, lanes


def lane_rotation(t=None):
    """64 found tuples with distinct indices, rotated by one lane per slice for 64 slices."""
    t = t or rotation64()
    qs = t.queries[:64]
    assert len(qs) == 64
    return [[(qs[(lane + r) % 64], _flags(lane, r)) for lane in range(64)] for r in range(64)]


def partial(t):
    """Five bursts: two full slices and a last one of 1, 3, 4, 5, 63 frames whose last valid lane
    walks (tables without a walker: looks up their last query)."""
    w = t.walkers or t.queries[-1:]
    out = []
    for k, n in enumerate(PARTIAL_SIZES):
        last = _still_slice(t, 2 + k, n) if t.still else [(t.queries[i % len(t.queries)], ACK) for i in range(n)]
        last[n - 1] = (w[k % len(w)], ACK)
        full = [_all_queries_slice(t, k), _all_queries_slice(t, k + 7)]
        out.append(full + [last])
    return out


def _all_queries_slice(t, s):
    qs = t.queries
    return [(qs[(lane + 5 * s) % len(qs)], _flags(lane, s)) for lane in range(64)]


def every_query(t):
    """One burst in which every query of the table sits on several lanes with and without SYN."""
    n = max(2, -(-3 * len(t.queries) // 64))
    return [_all_queries_slice(t, s) for s in range(n)]


def layouts(t):
    """name -> list of bursts, for the layouts this table supports."""
    out = {"every_query": [every_query(t)], "partial": partial(t)}
    if t.walkers and t.still:
        out["lane_walkers"] = [lane_walkers(t)[0]]
    if t.name == "rotation64":
        out["lane_rotation"] = [lane_rotation(t)]
    return out


def padded(burst, nslices):
    """The burst repeated until it has at least nslices slices (DEEP launches)."""
    out = list(burst)
    while len(out) < nslices:
        out += burst
    return out


# ------------------------------------------------------------------------ cache stream ---

def _flip(q, word, bit):
    """q with one bit of one key word flipped (dst: of the wire address, which flips one bit of
    the raw word pass 1 compares)."""
    return q._replace(label=f"{q.label}^{word}{bit}", kind=None, **{word: getattr(q, word) ^ (1 << bit)})


def _trunc40(q, small, n):
    return q_frame(q, small, n)[:40]


def _badck(q, small, n):
    f = bytearray(q_frame(q, small, n))
    f[50] ^= 0x40
    return bytes(f)


def cache_steps(t=None):
    """The per-wave sequence of steps (each a 64-entry slice) of cache_stream, with a name each.
    Lane l's base tuple cycles through exact hit / listener / no PCB / listener behind a NULL
    slot (cache_table)."""
    t = t or cache_table()
    base = []
    for lane in range(64):
        j = lane // 4 % 16
        base.append(t.q([f"base{j}", f"miss80_{j}", f"miss9998_{j}", f"miss8080_{j}"][lane % 4]))
    B = lambda fl=ACK: [(q, fl) for q in base]
    kinds = ["udp", "arp", "l2"]
    steps = [("no_tcp", [("other", kinds[lane % 3]) for lane in range(64)]),
             ("zero_first", [(ZERO_Q, ACK)] * 64), ("zero_again", [(ZERO_Q, SYN)] * 64),
             ("base", B()), ("same", B()), ("syn", B(SYN)), ("nosyn", B()), ("syn2", B(SYN))]
    for word in ("sport", "dport", "src", "dst"):
        for bit, what in ((0, "present"), (1, "absent")):
            steps.append((f"base_before_{word}_{what}", B()))
            steps.append((f"onebit_{word}_{what}", [(_flip(q, word, bit), ACK) for q in base]))
    for k in range(4):
        steps.append((f"base_before_between{k}", B()))
        sl = []
        for lane, q in enumerate(base):
            kind = (lane + k) % 4
            if kind < 2:
                sl.append(("other", kinds[kind]))
            elif kind == 2:
                sl.append(("raw", _trunc40(q, True, lane), _trunc40(q, False, lane)))
            else:
                sl.append(("raw", _badck(q, True, lane), _badck(q, False, lane)))
        steps.append((f"between{k}", sl))
    steps.append(("base_after_between", B()))
    for lane in (0, 37, 63):
        sl = B()
        sl[lane] = (base[(lane + 5) % 64], ACK)
        steps.append((f"all_but_{lane}", sl))
        steps.append((f"base_after_{lane}", B()))
    return steps


def zero_steps(t):
    """A short stream for the zero_tuple tables: no TCP frame first, then the all-zero tuple on
    every lane against the cache's initial (all-zero, invalid) key words, again with SYN, another
    tuple, and the zero tuple once more."""
    kinds = ["udp", "arp", "l2"]
    other = [q for q in t.queries if q.label != "zero"]
    return [("no_tcp", [("other", kinds[lane % 3]) for lane in range(64)]),
            ("zero_first", [(t.q("zero"), ACK)] * 64), ("zero_again", [(t.q("zero"), SYN)] * 64),
            ("others", [(other[lane % len(other)], ACK) for lane in range(64)]),
            ("zero_back", [(t.q("zero"), ACK)] * 64), ("zero_same", [(t.q("zero"), ACK)] * 64)]


def cache_stream(nwaves, steps=None):
    """Each step laid down nwaves times in a row: on a grid of nwaves waves, wave w takes slices
    w, w + nwaves, ..., so every wave meets every step once, in order."""
    steps = steps or cache_steps()
    return [sl for _, sl in steps for _ in range(nwaves)]


def stream_small_fn(nwaves):
    """Size forms of a stream go by step, in pairs (small, small, class, class, ...), so a cache
    entry written by either probe form is read after either."""
    def fn(form, s):
        return form == "small" or (form == "alt" and (s // nwaves) % 4 < 2)
    return fn


# --------------------------------------------------------------------------------- ARP ---

def arp_cluster(nb, with_zero):
    """An ARP mirror of nb buckets (4 or 16) with a cluster across the table's end.  The mirror is
    built in list order, so every address's place is known.  Returns a dict: known (in add_mac
    order, 0.0.0.0 first when with_zero), walk_found / walk_miss (lookups that leave their home
    bucket), still (those that do not; 0.0.0.0 among them), and later (addresses to learn)."""
    mask = nb - 1
    if nb == 4:
        clus = arp_addresses(mask, 3, 6)              # bucket 3 full, two in 0
        rest = arp_addresses(mask, 0, 1 if with_zero else 2)   # three (or four) in 0: eight addresses in all
        spare = []
    else:
        clus = arp_addresses(mask, 15, 14)            # 15, 0, 1 full, two in 2
        rest = [ip for h in (5, 6, 7, 8) for ip in arp_addresses(mask, h, 1)]
        spare = arp_addresses(mask, 9, 1 if with_zero else 2)
    known = ([0] if with_zero else []) + clus + rest + spare
    assert arp_nb(len(known)) == nb, (nb, len(known))
    occ = occupancy([arp_hash(ip) & mask for ip in known if ip], nb)
    miss = arp_addresses(mask, mask, 6, start=4000, avoid=known)
    assert miss_probes(occ, mask) >= 2
    still_miss = arp_addresses(mask, 2 if nb == 4 else 11, 3, start=4000, avoid=known)
    later = miss[:2] if nb == 16 else []   # (nb = 4 holds eight addresses already: a ninth rebuilds)
    return dict(nb=nb, known=known, walk_found=clus[4:], walk_miss=miss, still=clus[:4] + rest + still_miss + [0],
                later=later, zero=with_zero)


def arp_burst(a):
    """Four slices: ARP walkers on lanes 0, 31, 32, 63 only, every lane walking, the even lanes,
    and a slice of lookups that stay in their bucket (0.0.0.0 among them)."""
    w = a["walk_found"] + a["walk_miss"]
    st = a["still"]

    def e(ip, lane):
        return (Q(f"arp{ip:08x}", ip, 2000 + lane, 80, DST, "listen", None), SYN if lane % 2 else ACK)
    s0 = [e(st[lane % len(st)], lane) for lane in range(64)]
    for k, lane in enumerate((0, 31, 32, 63)):
        s0[lane] = e(w[(3 * k) % len(w)], lane)
    s1 = [e(w[lane % len(w)], lane) for lane in range(64)]
    s2 = [e(w[lane % len(w)] if lane % 2 == 0 else st[lane % len(st)], lane) for lane in range(64)]
    s3 = [e(st[(lane + 1) % len(st)], lane) for lane in range(64)]
    return [s0, s1, s2, s3], [{0, 31, 32, 63}, set(range(64)), set(range(0, 64, 2)), set()]


ARP_TABLE_ROWS = [(80, 0, DST_RAW, 0, LISTENING)]


# ----------------------------------------------------------------- the check program's file ---

def check_file_text(t=None, queries=None, arp=None, arp_queries=(), load_only=False):
    """The input of tests/lookup_check.cpp for a table (its ops as the writes) and / or an ARP
    set."""
    out = []
    if t is not None:
        out.append(f"T {len(t.rows)}")
        for r in t.rows:
            out.append(" ".join(str(int(x) & M32) for x in (r or (0, 0, 0, 0, 0))) + (" 0" if r is None else " 1"))
        ops = [] if load_only else t.ops
        out.append(f"W {len(ops)}")
        for op in ops:
            out.append(f"0 {op[1]}" if op[0] == "remove" else f"1 {op[1]} " + " ".join(str(int(x) & M32) for x in op[2]))
        qs = t.queries if queries is None else queries
        out.append(f"Q {len(qs)}")
        out += [" ".join(str(w) for w in key_of(q)) for q in qs]
    if arp is not None:
        out.append(f"A {len(arp['known'])}")
        out += [str(ip) for ip in arp["known"]]
        out.append(f"L {len(arp['later'])}")
        out += [str(ip) for ip in arp["later"]]
        out.append(f"R {len(arp_queries)}")
        out += [str(ip) for ip in arp_queries]
    return "\n".join(out) + "\n"
