"""Deterministic cases for the device planner (rxg_tx_plan_dev, csrc/rxg_txplan.hip): send counts on
both sides of every tile and scan-round edge, segment counts that put a send's first and last
segment on the edges of the expand pass's 64-segment slices, every flag combination, the 32-bit
wraps, 64-bit offsets, option blocks, refused sends, `cap`, and the NULL arguments.

The reference is the shipped host planner, called through the binding (rxg.tx_plan_opt), on the
sends that are not refused (it answers a refused one with -EINVAL); first[] and count come from
the per-send segment counts, and expect() holds them against the planner's own output (segment 0
of every send carries the send's next_seq and src_off).  tests/test_txplan_cases_host.py holds
every claim made below against the sets themselves.
"""
from __future__ import annotations

import numpy as np

import rxg

# csrc/rxg_txplan.hip: tx_plan_count takes a lane per send and a workgroup per tile of kTile = 256
# sends, a wave per 64 of them; tx_plan_scan is one workgroup of kScanLanes = 1024 lanes, a tile
# per lane, so a round of its loop covers 1024 tiles; tx_plan_expand takes a wave per 64
# consecutive segment indices.
SLICE = 64
TILE = 256
SCAN_WAVE = 64 * TILE
SCAN_ROUND = 1024 * TILE

FILL = 0xA5
GUARD = 8           # descriptors / entries behind the end that must keep their fill
MSS = 1460
SYN, FIN, PSH, ACK = rxg.TCP_FLAG_SYN, rxg.TCP_FLAG_FIN, rxg.TCP_FLAG_PSH, rxg.TCP_FLAG_ACK

# blocks 1..6: len 0, 4, 12, 40 (valid), 44 and 6 (refused); index 7 = nopts + 1 (refused)
OPT_LENS = (0, 4, 12, 40, 44, 6)
K_NONE, K_O0, K_O4, K_O12, K_O40, K_LEN44, K_LEN6, K_PAST = range(8)
GOOD = (K_NONE, K_O0, K_O4, K_O12, K_O40)


def make_opts() -> np.ndarray:
    """The block table: garbage everywhere but in `len`."""
    raw = np.random.default_rng(48).integers(0, 256, (len(OPT_LENS), 48), dtype=np.uint8)
    raw[:, 0] = OPT_LENS
    return np.ascontiguousarray(raw).view(rxg.TX_OPT_DTYPE).reshape(-1)


OPTS = make_opts()


def make_sends(nbytes, seed, flags=None, next_seq=None, src_off=None, ip_id0=None) -> np.ndarray:
    """One send per entry of nbytes; every other field seeded random (the pad bytes too)."""
    nbytes = np.asarray(nbytes, dtype=np.uint64)
    n = nbytes.size
    r = np.random.default_rng(seed)
    raw = r.integers(0, 256, (n, rxg.TX_SEND_DTYPE.itemsize), dtype=np.uint8)
    s = np.ascontiguousarray(raw).view(rxg.TX_SEND_DTYPE).reshape(-1)
    s["bytes"] = nbytes.astype(np.uint32)
    s["src_off"] = r.integers(0, 1 << 44, n, dtype=np.uint64) if src_off is None else src_off
    s["tcp_flags"] = r.integers(0, 32, n, dtype=np.uint8) if flags is None else flags
    if next_seq is not None:
        s["next_seq"] = next_seq
    if ip_id0 is not None:
        s["ip_id0"] = ip_id0
    return s


def case(name, sends, mss=MSS, send_opt=None, cap=("total", 0), next_seq=True, opts=OPTS):
    so = None if send_opt is None else np.ascontiguousarray(send_opt, dtype=np.uint32)
    assert so is None or len(so) == len(sends)
    return dict(name=name, sends=sends, mss=mss, send_opt=so, opts=opts, cap=cap, next_seq=next_seq)


# -------------------------------------------------------------------------------- model ---
def block_of(c) -> np.ndarray:
    return np.zeros(len(c["sends"]), np.uint32) if c["send_opt"] is None else c["send_opt"]


def _block_len(c):
    """(send_opt[j] > nopts, the len of the block send j names or 0), int64."""
    k, opts = block_of(c).astype(np.int64), c["opts"]
    past = k > len(opts)
    lens = opts["len"].astype(np.int64) if len(opts) else np.zeros(1, np.int64)
    return past, np.where((k > 0) & ~past, lens[np.clip(k - 1, 0, len(lens) - 1)], 0)


def refused(c) -> np.ndarray:
    """The rule of include/rxg.h: send_opt[j] > nopts, len over 40 or not a multiple of 4, mss <= O."""
    past, O = _block_len(c)
    return past | (O > 40) | ((O & 3) != 0) | (c["mss"] <= O)


def cut(c) -> np.ndarray:
    """m_j per send (0 where refused)."""
    return np.where(refused(c), 0, c["mss"] - _block_len(c)[1]).astype(np.int64)


def nseg(c) -> np.ndarray:
    m, b = cut(c), c["sends"]["bytes"].astype(np.int64)
    return np.where(m == 0, 0, np.where(b == 0, 1, -(-b // np.maximum(m, 1)))).astype(np.uint64)


def first_of(c) -> np.ndarray:
    f = np.zeros(len(c["sends"]) + 1, np.uint64)
    np.cumsum(nseg(c), out=f[1:])
    return f


def cap_of(c) -> int:
    first = first_of(c)
    kind = c["cap"]
    if isinstance(kind, tuple) and kind[0] == "total":
        return int(first[-1]) + kind[1]
    if isinstance(kind, tuple) and kind[0] == "first":
        return int(first[kind[1]]) + kind[2]
    return int(kind)


_memo: dict = {}


def expect(c) -> dict:
    """What the call must leave in its four buffers, each pre-filled with FILL and carrying GUARD
    entries behind its end: segs u8[(cap + GUARD) * 32], first u64[nsends + 1 + GUARD], next_seq
    u32[nsends + GUARD], count u64[2].  Computed once per case and shared (never written to)."""
    if c["name"] in _memo:
        return _memo[c["name"]]
    sends, n = c["sends"], len(c["sends"])
    ref = refused(c)
    keep = ~ref
    so = None if c["send_opt"] is None else c["send_opt"][keep]
    segs, nxt = rxg.tx_plan_opt(sends[keep], c["mss"], so, c["opts"])
    first, cap = first_of(c), cap_of(c)
    total = int(first[-1])
    assert total == len(segs) and cap >= 0
    # first[] against the planner's own output: segment 0 of a send is the send's start
    at = first[:-1][keep].astype(np.int64)
    assert np.array_equal(segs["seq"][at], sends["next_seq"][keep])
    assert np.array_equal(segs["src_off"][at], sends["src_off"][keep])
    w = dict(cap=cap, total=total, nrefused=int(ref.sum()))
    w["segs"] = np.full((cap + GUARD) * 32, FILL, np.uint8)
    nb = min(total, cap)
    w["segs"][:nb * 32] = segs[:nb].view(np.uint8).reshape(-1)
    w["first"] = np.full(n + 1 + GUARD, 0xA5A5A5A5A5A5A5A5, np.uint64)
    w["first"][:n + 1] = first
    w["next_seq"] = np.full(n + GUARD, 0xA5A5A5A5, np.uint32)
    if c["next_seq"]:
        w["next_seq"][:n][keep] = nxt
        w["next_seq"][:n][ref] = sends["next_seq"][ref]
    w["count"] = np.array([total, w["nrefused"]], np.uint64)
    for v in w.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _memo[c["name"]] = w
    return w


# -------------------------------------------------------------------------------- cases ---
def mixed(n, seed):
    """n sends of 0 .. 3 segments' worth of bytes with every block kind, a few of them refused."""
    r = np.random.default_rng(seed)
    so = r.choice(np.array(GOOD + (K_LEN44, K_LEN6, K_PAST), np.uint32), n,
                  p=[.3, .1, .15, .2, .15, .04, .03, .03])
    if n >= 8:  # every kind at least once
        so[r.permutation(n)[:8]] = np.arange(8)
    return make_sends(r.integers(0, 3 * MSS + 1, n), seed + 1), so


SEND_COUNTS = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, SCAN_WAVE - 1, SCAN_WAVE, SCAN_WAVE + 1)
ROUND_COUNTS = (SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1)


def send_count_cases():
    out = []
    for n in SEND_COUNTS:
        s, so = mixed(n, 100 + n)
        out.append(case(f"count_{n}", s, send_opt=so))
    for n in ROUND_COUNTS:  # one-segment sends, a three-segment one at each end and on the round's edge
        b = np.random.default_rng(n).integers(0, MSS + 1, n)
        b[[0, SCAN_ROUND - 2, n - 1]] = 2 * MSS + 1
        out.append(case(f"round_{n}", make_sends(b, 200 + n % 7)))
    return out


def byte_edge_cases():
    out = []
    for k in (K_NONE, K_O12):
        m = MSS - (OPT_LENS[k - 1] if k else 0)
        b = [0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1]
        out.append(case(f"bytes_edges_block{k}", make_sends(b, 300 + k), send_opt=np.full(len(b), k)))
    return out


LANE_MSS = 7
LANE_NSEG = (63, 64, 65)


def lane_case():
    """Sends of 63, 64 and 65 segments, each once with its first segment on lane 0 and on lane 63
    of an output slice and once with its last segment there (fillers of fewer segments between)."""
    ns, pos = [], 0
    for N in LANE_NSEG:
        for first_lane in (0, 63, (0 - (N - 1)) % 64, (63 - (N - 1)) % 64):
            fill = (first_lane - pos) % 64
            if fill:
                ns.append(fill)
                pos += fill
            ns.append(N)
            pos += N
    b = np.array(ns) * LANE_MSS - 3
    return case("lanes_63_64_65", make_sends(b, 400), mss=LANE_MSS)


BIG = (1 << 20) + 1


def big_cases():
    one = make_sends([BIG], 500)
    between = make_sends([1, 1, 1, BIG, 1, 1], 501)
    return [case("big_alone", one, mss=1), case("big_between", between, mss=1),
            case("one_segment_sends_2^16+1", make_sends(np.random.default_rng(5).integers(0, MSS + 1, (1 << 16) + 1), 502))]


def flag_case():
    fl, b = [], []
    for ns in (1, 2, 3):
        for combo in range(16):
            fl.append((SYN if combo & 1 else 0) | (FIN if combo & 2 else 0) | (PSH if combo & 4 else 0) |
                      (ACK if combo & 8 else 0))
            b.append(ns * MSS - 5)
    return case("flags_16x3", make_sends(b, 600, flags=np.array(fl, np.uint8)))


WRAP_NSEG = 4


def wrap_case():
    m = MSS
    b = [m * WRAP_NSEG - 9, m * WRAP_NSEG - 9, 5 * m, 10, 10]
    seq = [0xFFFFFFFF, (1 << 32) - m * WRAP_NSEG + 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFE]
    fl = [ACK, ACK | PSH, SYN | FIN, SYN | FIN, SYN | FIN]
    ids = [7, 8, 0xFFFE, 0xFFFF, 0]
    return case("wraps", make_sends(b, 700, flags=np.array(fl, np.uint8), next_seq=np.array(seq, np.uint32),
                                    ip_id0=np.array(ids, np.uint16)))


CARRY_OFF = (1 << 40) + (1 << 32) - 7   # low word 2^32 - 7: src_off + q * m carries into the high word


def offset_cases():
    """src_off 2^40 + 7; sends whose src_off + q * m carries out of the low word (from the second
    segment on, and in the 2^32 - 1 byte send from the first segment after segment 0); a src_off
    at the top of the 64-bit range."""
    a = make_sends([3 * MSS + 1, 3 * MSS + 1, 10], 800,
                   src_off=np.array([(1 << 40) + 7, CARRY_OFF, (1 << 64) - 1 - 5000], np.uint64))
    b = make_sends([1, (1 << 32) - 1, 1], 801, src_off=np.array([1, CARRY_OFF, 2], np.uint64))
    return [case("src_off_2^40+7", a), case("bytes_2^32-1", b, mss=rxg.TX_MAX_DATA)]


def block_case():
    so = np.array([K_NONE, K_O0, K_O4, K_O12, K_O40] * 13, np.uint32)[:64]
    r = np.random.default_rng(9)
    return case("blocks_in_one_slice", make_sends(r.integers(0, 2 * MSS, 64), 900), send_opt=so)


REFUSED_KINDS = (K_PAST, K_LEN44, K_LEN6)


def refused_cases():
    out = []
    # each kind alone among good sends; refused first, last and two in a row
    n = 10
    for name, where in (("first", [0]), ("last", [n - 1]), ("pair", [4, 5]), ("first_last_pair", [0, 3, 4, n - 1])):
        for kind in REFUSED_KINDS:
            so = np.array([GOOD[j % len(GOOD)] for j in range(n)], np.uint32)
            so[where] = kind
            out.append(case(f"refused_{name}_kind{kind}", make_sends(np.arange(n) * 700, 1000 + kind), send_opt=so))
    # mss == O: with mss 40 the sends of block 4 (len 40) are refused, the others cut at 40 - O
    so = np.array([K_O40, K_NONE, K_O12, K_O40, K_O40, K_O4, K_O40], np.uint32)
    out.append(case("refused_mss_eq_O", make_sends([100, 100, 100, 0, 5, 90, 1], 1010), mss=40, send_opt=so))
    # refused on lanes 0, 31, 32 and 63 of a wave of the count pass (and of the second tile's first wave)
    so = np.zeros(TILE + 64, np.uint32)
    for base in (0, 64, TILE):
        so[[base, base + 31, base + 32, base + 63]] = [K_PAST, K_LEN44, K_LEN6, K_PAST]
    out.append(case("refused_lanes", make_sends(np.random.default_rng(3).integers(0, 3 * MSS, TILE + 64), 1020),
                    send_opt=so))
    # every send refused
    out.append(case("refused_all", make_sends(np.arange(70) * 100, 1030),
                    send_opt=np.array([REFUSED_KINDS[j % 3] for j in range(70)], np.uint32)))
    return out


def cap_cases():
    s, so = mixed(150, 1100)
    out = [case(f"cap_total{d:+d}", s, send_opt=so, cap=("total", d)) for d in (0, -1)]
    out.append(case("cap_0", s, send_opt=so, cap=0))
    j = 77  # a send of more than one segment that is not refused (asserted in the host test)
    so = so.copy()
    so[j] = K_O12
    s = s.copy()
    s["bytes"][j] = 3 * (MSS - 12)
    out += [case(f"cap_first{d:+d}", s, send_opt=so, cap=("first", j, d)) for d in (0, 1)]
    return out


CAP_SEND = 77


def null_cases():
    s, so = mixed(130, 1200)
    return [case("send_opt_null", s, send_opt=None), case("next_seq_null", s, send_opt=so, next_seq=False),
            case("opts_null", s, send_opt=None, opts=np.zeros(0, rxg.TX_OPT_DTYPE))]


def all_cases():
    out = (send_count_cases() + byte_edge_cases() + [lane_case()] + big_cases() + [flag_case(), wrap_case()] +
           offset_cases() + [block_case()] + refused_cases() + cap_cases() + null_cases())
    assert len({c["name"] for c in out}) == len(out)
    return out


SMALL = 1 << 15     # cases of at most this many sends and segments run in the parametrised GPU test


def size_of(c) -> int:
    return max(len(c["sends"]), int(first_of(c)[-1]))
