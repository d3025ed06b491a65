"""Deterministic sets for the option segment build (rxg_tx_build_opt_dev, tx_build_kernel<true>
in csrc/rxg_txbuild.hip): what the option instantiation has and the plain one has not -- the
second byte mask (drop_bytes, the frame bytes before H = 54 + O), the block's chunks ORed into
frame chunks 3, 4 and 5, the source clamp as 32-bit offsets from the first source chunk,
streamed frames without data, the one-line path that loads a block chunk, a size class that
depends on O + L and the block index carried in the group broadcast -- at every block length
O = 0, 4, .. 40 (txbuild_opt_ref.ALL_OPT_LENS; 20, 24, 32 and 36 run nowhere else).

Every set is a Case: (payload, flows, segs, opts, off64, nslots) and the labels the host file
(tests/test_txbuild_opt_cases_host.py) holds the set's claims against.  Expectations come from
txbuild_opt_ref.build (Case.model), the oracle's checksums, never from the kernel.  numpy
only; nothing here touches a GPU.

  masks(O)            every tail residue x every source shift on two-line frames; every
                      data_len 0..48 x every source alignment
  class_edges()       payload_lengths(O) x alignments for every O, blocks made of real options;
                      slice 0 holds one data_len under O = 16, 20, 24 across a class edge
  slices(cls)         two full slices and a partial one of one size class, O mixed
  slices_all()        those full slices, the four geometry slices and a partial one, one batch
  surroundings(f, O)  0xFF inside / 0x00 outside and the reverse, block garbage included
  single_bytes()      40 blocks of 40 bytes whose byte j alone is 0xFF
  payload_starts(O)   src_off 0..15: the first source chunk up to 48 bytes before the buffer
  payload_ends(pb)    segments ending exactly at payload_bytes, 0xEE behind it
  longest(O)          RXG_TX_MAX_DATA - O on both sides of the shift's zero
  checksums()         stored checksums of 0x0000, the largest sum, a sum that carries twice
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import rxg
import rxopt_cases as rxc
import txbuild_opt_ref as oref
import txbuild_ref as ref

HDR = oref.HDR
ALL = oref.ALL_OPT_LENS
FILL = 0xA5
LIMIT = 1 << 20          # no committed file is larger; no set's pool is either
SMALL_MAX = 2731         # data_len stays at or below this except in longest() and checksums()
LONG_ALIGN = [0, 5, 6, 11, 15]
CLASSES = ref.CLASSES
# class -> (fewest, most) frame bytes H + L (csrc/rxg_txbuild.hip class_of)
HL_RANGE = {0: (HDR, 64), 4: (65, 256), 8: (257, 512), 16: (513, 1024), 32: (1025, 2048),
            64: (2049, HDR + SMALL_MAX)}
SIX_COUNTS = {64: 1, 32: 3, 16: 5, 8: 9, 4: 17, 0: 29}
SKIP_LANES = {0: "index", 31: "len 44", 32: "len 6", 63: "data_len"}


@dataclass
class Case:
    payload: np.ndarray
    flows: np.ndarray
    segs: np.ndarray
    opts: np.ndarray
    off64: np.ndarray
    nslots: int
    nopts: int | None = None          # the bound passed (default: the whole table)
    payload_bytes: int | None = None  # the bound passed (default: the whole buffer)
    labels: dict = field(default_factory=dict)

    @property
    def args(self):
        return self.payload, self.flows, self.segs, self.opts, self.off64, self.nslots

    @property
    def kw(self):
        """What the GPU tests' check() and run_opt() take beside args."""
        out = {}
        if self.nopts is not None:
            out["nopts"] = self.nopts
        if self.payload_bytes is not None:
            out["payload_bytes"] = self.payload_bytes
        return out

    def model(self, fill=FILL):
        pb = len(self.payload) if self.payload_bytes is None else self.payload_bytes
        return oref.build(self.payload[:pb], self.flows, self.segs, self.opts, self.off64, self.nslots, fill=fill,
                          nopts=self.nopts)

    def opt_len(self):
        return oref.opt_len(self.segs, self.opts, self.nopts)


def block_of(O):
    """The index + 1 (rxg_tx_seg.reserved) of the block of O bytes in table()."""
    return O // 4 + 1


def table(seed=21):
    """One block per length, block_of(O) its index + 1; random option bytes and random bytes
    in everything the call must ignore."""
    return oref.make_opts(ALL, seed)


def cls_of(O, L):
    return ref.lanes_per_frame(int(O) + int(L))


def one_per_class(O):
    """One data_len per size class behind a block of O bytes: test_gpu_txbuild_classes's
    ONE_PER_CLASS less O (the same frame bytes), the one-line class while it exists (O <= 8)."""
    small = [7 - O if O <= 4 else 1] if O <= 8 else []
    return small + [x - O for x in (139, 331, 715, 1483, 2731)]


def _pack(dl, ol, r, spare=2, skipped=None):
    """Slots back to back in a random order; a skipped descriptor gets one slot."""
    tot = np.asarray(dl, dtype=np.int64) + np.asarray(ol, dtype=np.int64)
    if skipped is not None:
        tot = np.where(skipped, 0, tot)
    off, nslots = ref.packed_offsets(tot, r.permutation(len(tot)))
    return off, nslots + spare


# ----------------------------------------------------------------------------- masks ---
def mask_rows(O):
    """(data_len, src_off mod 16) of masks(O): rows 0..255 the residue x shift grid on the
    smallest streamed frames with data that have the residue, rows 256.. every data_len 0..48
    at every alignment."""
    H = HDR + O
    rows = []
    for res in range(16):
        HL = next(x for x in range(max(65, H + 1), 129) if x % 16 == res)
        rows += [(HL - H, (sh - 10 + O) % 16) for sh in range(16)]
    rows += [(L, a) for L in range(49) for a in range(16)]
    return rows


def masks(O):
    rows = mask_rows(O)
    n = len(rows)
    r = np.random.default_rng(1000 + O)
    payload = np.random.default_rng(7).integers(0, 256, 8192, dtype=np.uint8)
    dl = np.array([x[0] for x in rows])
    al = np.array([x[1] for x in rows])
    flows = ref.make_flows(8)
    segs = ref.make_segs(dl, r.integers(0, (len(payload) - 64) // 16, n) * 16 + al, len(flows), seed=1100 + O)
    segs["reserved"] = block_of(O)
    if O == 0:  # no block at all on about half of them, the block of no bytes on the others
        segs["reserved"][r.random(n) < 0.5] = 0
    off, nslots = _pack(dl, np.full(n, O), r)
    return Case(payload, flows, segs, table(), off, nslots, labels=dict(O=O, stride64=3))


# ----------------------------------------------------------------------- class_edges ---
_TS = rxc.aligned_ts(0x01020304, 0xA0B0C0D0)
REAL_OPTIONS = {
    0: b"",
    4: rxc.mss(1460),
    8: rxc.mss(536) + rxc.NOP + rxc.wscale(7),
    12: _TS,
    16: _TS + rxc.mss(1448),
    20: rxc.timestamp(203032, 0) + rxc.mss(1300) + rxc.wscale(7) + rxc.EOL * 3,
    24: rxc.mss(1460) + rxc.sack_perm() + rxc.timestamp(0xCAFE0001, 0) + rxc.NOP + rxc.wscale(9) + rxc.NOP * 4,
    28: _TS + rxc.NOP * 2 + rxc.sack(1) + rxc.mss(9000),
    32: _TS + rxc.NOP * 2 + rxc.sack(2),
    36: _TS + rxc.NOP * 2 + rxc.sack(2) + rxc.mss(1220),
    40: _TS + rxc.NOP * 2 + rxc.sack(3),
}


def real_table(seed=22):
    """table() with each block's bytes [0, O) real TCP options (what follows stays random)."""
    o = table(seed)
    for O, b in REAL_OPTIONS.items():
        assert len(b) == O
        o[block_of(O) - 1]["bytes"][:O] = np.frombuffer(b, np.uint8)
    return o


EDGES = (256, 512, 1024)
EDGE_ALIGN = (0, 1, 5, 6, 10, 11, 15)


def edge_rows():
    """(O, data_len, src_off mod 16) of class_edges(); the first 64 are the shared slice: at
    each edge E one data_len, E - 74, under O = 16, 20 and 24 (H + L = E - 4, E, E + 4)."""
    rows = [(O, E - 74, a) for E in EDGES for O in (16, 20, 24) for a in EDGE_ALIGN] + [(0, 0, 0)]
    assert len(rows) == 64
    for O in ALL:
        for L in oref.payload_lengths(O):
            rows += [(O, L, a) for a in (range(16) if L <= 300 else LONG_ALIGN)]
    return rows


def class_edges():
    rows = edge_rows()
    n = len(rows)
    r = np.random.default_rng(2000)
    payload = np.random.default_rng(11).integers(0, 256, 1 << 17, dtype=np.uint8)
    ol, dl, al = (np.array([x[k] for x in rows]) for k in range(3))
    flows = ref.make_flows(8)
    segs = ref.make_segs(dl, r.integers(0, (len(payload) - SMALL_MAX - 16) // 16, n) * 16 + al, len(flows), seed=2001)
    segs["reserved"] = ol // 4 + 1
    segs["reserved"][(ol == 0) & (r.random(n) < 0.5)] = 0
    off, nslots = _pack(dl, ol, r)
    return Case(payload, flows, segs, real_table(), off, nslots, labels=dict(O=ol))


# ---------------------------------------------------------------------------- slices ---
N_EXTRA = 64
K_LEN44, K_LEN6, K_LAST, K_PAST = 76, 77, 78, 79
SLICE_NOPTS = K_LAST


def slice_table(seed=23):
    """79 blocks: 1..11 table()'s, 12..75 of lengths 4, 8, .. 40 in turn, 76 of `len` 44, 77 of
    `len` 6, 78 the last inside the bound passed (SLICE_NOPTS), 79 a good block beyond it."""
    lens = list(ALL) + [ALL[1 + j % 10] for j in range(N_EXTRA)] + [44, 6, 12, 8]
    assert len(lens) == K_PAST
    return oref.make_opts(lens, seed)


def _draw(r, cls, n, turn=0):
    """n (reserved, data_len) of one size class, O taking every length the class has in turn
    and both ends of the class among them."""
    lo, hi = HL_RANGE[cls]
    allowed = [O for O in ALL if HDR + O <= hi and (cls or O <= 8)]
    ol = np.array([allowed[(turn + i) % len(allowed)] for i in range(n)])
    low = np.maximum(lo, HDR + ol)
    hl = r.integers(low, hi + 1)
    if n >= 2:
        at = r.choice(n, 2, replace=False)
        hl[at[0]], hl[at[1]] = low[at[0]], hi
    kk = ol // 4 + 1
    kk[(ol == 0) & (r.random(n) < 0.5)] = 0
    return kk, hl - HDR - ol


def _assemble(parts, seed, names):
    r = np.random.default_rng(seed)
    kk = np.concatenate([p[0] for p in parts])
    dl = np.concatenate([p[1] for p in parts])
    n = len(kk)
    opts = slice_table()
    payload = np.random.default_rng(11).integers(0, 256, 1 << 17, dtype=np.uint8)
    flows = ref.make_flows(8)
    segs = ref.make_segs(dl, r.integers(0, len(payload) - rxg.TX_MAX_DATA - 1, n), len(flows), seed=seed + 1)
    segs["reserved"] = kk
    skip = oref.skipped(segs, len(flows), len(payload), opts, SLICE_NOPTS)
    ol = np.maximum(oref.opt_len(segs, opts, SLICE_NOPTS), 0)
    off, nslots = _pack(dl, ol, r, skipped=skip)
    return Case(payload, flows, segs, opts, off, nslots, nopts=SLICE_NOPTS, labels=dict(names=names, O=ol, skipped=skip))


def slices(cls):
    """Two full slices of one class (every lane builds: no lane compaction) and one of 17."""
    r = np.random.default_rng(3000 + cls)
    return _assemble([_draw(r, cls, 64), _draw(r, cls, 64, 3), _draw(r, cls, 17, 5)], 3100 + cls, ["full", "full", "17"])


def _six(r):
    """Per-class counts that end inside a round of 64 / LPF frames, lanes interleaved."""
    parts = [_draw(r, c, k, turn=c) for c, k in SIX_COUNTS.items()]
    kk, dl = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    p = r.permutation(64)
    return kk[p], dl[p]


def _blocks(r, same):
    """64 lanes naming 64 different blocks (12..75), or all the last block inside the bound."""
    kk = np.full(64, K_LAST) if same else 12 + r.permutation(N_EXTRA)
    dl = r.choice([0, 1, 9, 30, 139, 200, 331, 715], 64)
    return kk, dl


def _skips(r):
    kk, dl = _six(r)
    for lane, k in ((0, K_PAST), (31, K_LEN44), (32, K_LEN6)):
        kk[lane] = k
    kk[63], dl[63] = block_of(40), rxg.TX_MAX_DATA - 40 + 1
    return kk, dl


def slices_all():
    """One batch for the capped grids: 12 full slices of one class each, the slice of all six
    classes, of 64 different blocks, of one block, of skipped descriptors, and one of 17."""
    r = np.random.default_rng(3500)
    parts, names = [], []
    for cls in CLASSES:
        parts += [_draw(r, cls, 64, 1), _draw(r, cls, 64, 7)]
        names += [f"class {cls}"] * 2
    parts += [_six(r), _blocks(r, False), _blocks(r, True), _skips(r)]
    names += ["six", "different blocks", "same block", "skips"]
    tail = _six(r)
    parts.append((tail[0][:17], tail[1][:17]))
    names.append("17")
    return _assemble(parts, 3600, names)


# ---------------------------------------------------------------------- surroundings ---
FORMS = [(0xFF, 0x00), (0x00, 0xFF)]


def surroundings(inside, outside, O):
    """Every segment's bytes and its block's bytes [0, O) are `inside`; every other payload
    byte, the block's bytes [O, 40) and the reserved fields of every block are `outside`."""
    lens = np.repeat(one_per_class(O), 16)
    align = np.tile(np.arange(16), len(lens) // 16)
    so, cursor = [], 0
    for L, a in zip(lens, align):  # 64 bytes of `outside` on both sides: the first source chunk lies up to 48 before
        so.append(cursor + 64 + int(a))
        cursor += 64 + (int(a) + int(L) + 15) // 16 * 16 + 64
    payload = np.full(cursor, outside, np.uint8)
    for L, o in zip(lens, so):
        payload[o:o + int(L)] = inside
    opts = np.full(len(ALL) * 48, outside, np.uint8).view(rxg.TX_OPT_DTYPE)
    opts["len"] = ALL
    for k, x in enumerate(ALL):
        opts[k]["bytes"][:x] = inside
    flows = ref.make_flows(8)
    segs = ref.make_segs(lens, np.array(so), len(flows), seed=4000 + O + inside)
    segs["reserved"] = block_of(O)
    off, nslots = _pack(lens, np.full(len(lens), O), np.random.default_rng(4100 + O))
    return Case(payload, flows, segs, opts, off, nslots, labels=dict(O=O, inside=inside, outside=outside))


def single_bytes():
    """41 segments alike but for their block: block 1 is 40 zero bytes, block 2 + j has byte j
    alone 0xFF (what the call must ignore: 0xFF in all of them), over a zero payload."""
    opts = np.zeros(41, dtype=rxg.TX_OPT_DTYPE)
    opts["reserved0"], opts["reserved1"], opts["len"] = 0xFF, 0xFF, 40
    for j in range(40):
        opts[1 + j]["bytes"][j] = 0xFF
    dl = np.full(41, 21)
    flows = ref.make_flows(8)
    segs = ref.make_segs(dl, np.full(41, 3), len(flows), seed=4200)
    for f in ("flow", "seq", "ack", "win_raw", "ip_id", "tcp_flags"):
        segs[f] = segs[f][0]
    segs["reserved"] = 1 + np.arange(41)
    off, nslots = _pack(dl, np.full(41, 40), np.random.default_rng(4201))
    return Case(np.zeros(64, np.uint8), flows, segs, opts, off, nslots)


# ---------------------------------------------------------------------- payload ends ---
def payload_starts(O):
    lens = np.repeat(one_per_class(O), 16)
    payload = np.random.default_rng(5000).integers(0, 256, 4096, dtype=np.uint8)
    flows = ref.make_flows(8)
    segs = ref.make_segs(lens, np.tile(np.arange(16), len(lens) // 16), len(flows), seed=5001 + O)
    segs["reserved"] = block_of(O)
    off, nslots = _pack(lens, np.full(len(lens), O), np.random.default_rng(5002 + O))
    return Case(payload, flows, segs, table(), off, nslots, labels=dict(O=O))


END_BYTES = [4096, 4097, 4107]
SLACK = 0xEE


def payload_ends(pbytes):
    """Every payload_lengths(O) length of every O ending exactly at payload_bytes (data_len
    0: src_off == payload_bytes).  From there to the buffer's end SLACK, which neither the
    data nor the option bytes hold."""
    data = np.random.default_rng(pbytes).integers(0, 256, pbytes, dtype=np.uint8)
    data[data == SLACK] = 0x11
    buf = np.concatenate([data, np.full(16 - pbytes % 16, SLACK, np.uint8)])
    opts = table()
    b = opts["bytes"]
    b[b == SLACK] = 0x11
    rows = [(O, L) for O in ALL for L in oref.payload_lengths(O)]
    ol, dl = np.array([x[0] for x in rows]), np.array([x[1] for x in rows])
    flows = ref.make_flows(8)
    segs = ref.make_segs(dl, pbytes - dl, len(flows), seed=pbytes + 1)
    segs["reserved"] = ol // 4 + 1
    off, nslots = _pack(dl, ol, np.random.default_rng(pbytes + 2))
    return Case(buf, flows, segs, opts, off, nslots, payload_bytes=pbytes, labels=dict(O=ol))


def longest(O):
    """RXG_TX_MAX_DATA - O twice: the source shift (src_off + 10 - O) mod 16 zero, and 5."""
    L = rxg.TX_MAX_DATA - O
    payload = np.random.default_rng(5500 + O).integers(0, 256, rxg.TX_MAX_DATA + 32, dtype=np.uint8)
    so = np.array([(O - 10) % 16, (O - 10) % 16 + 5])
    flows = ref.make_flows(8)
    segs = ref.make_segs(np.array([L, L]), so, len(flows), seed=5501 + O)
    segs["reserved"] = block_of(O)
    off, nslots = _pack([L, L], [O, O], np.random.default_rng(5502 + O), spare=1)
    return Case(payload, flows, segs, table(), off, nslots, labels=dict(O=O))


# ------------------------------------------------------------------------- checksums ---
def tcp_sum32(frame, flen, zero_field=True):
    """The unfolded sum the device forms: the 16-bit little-endian words of the pseudo header
    and of the TCP segment frame[34, flen), the checksum field taken as zero."""
    f = bytearray(bytes(frame[:flen]))
    if zero_field:
        f[50:52] = b"\0\0"
    b = bytes(f[26:34]) + bytes([0, 6]) + (flen - 34).to_bytes(2, "big") + bytes(f[34:])
    if len(b) % 2:
        b += b"\0"
    return int(np.frombuffer(b, "<u2").astype(np.int64).sum())


ZERO_TCP = [  # (size class, O, frame offset of the free option word): chunk 3, 4, 5, each twice
    (0, 8, 56), (4, 24, 70), (8, 40, 90), (16, 8, 56), (32, 24, 70), (64, 40, 90)]
I_IP, I_MAX, I_CARRY = 6, 7, 8


def checksums():
    """Segments 0-5: one per size class whose stored TCP checksum is 0x0000, the free word an
    option word of frame chunk 3 (O = 8), 4 (O = 24), 5 (O = 40).  6: an IP header checksum of
    0x0000 under O = 20.  7: the largest sum -- 40 option bytes and RXG_TX_MAX_DATA - 40
    payload bytes of 0xFF, every header field all ones.  8: a sum that still carries after one
    fold.  The free words are found with the model, as test_stored_checksums_of_zero finds
    them: with the word zero the stored field is the complement of the folded sum S of the
    rest, and S + ~S = 0xFFFF, so the word wanted is that field's two bytes."""
    ol = np.array([x[1] for x in ZERO_TCP] + [20, 40, 12])
    hl = [63, 193, 385, 769, 1537, 2785]
    dl = np.array([h - HDR - O for h, (_, O, _) in zip(hl, ZERO_TCP)] + [100, rxg.TX_MAX_DATA - 40, 1400])
    n = len(dl)
    opts = oref.make_opts(ol.tolist(), seed=6000)
    opts[I_MAX]["bytes"][:40] = 0xFF
    flows = np.concatenate([ref.make_flows(8), np.full(32, 0xFF, np.uint8).view(rxg.TX_FLOW_DTYPE)])
    payload = np.random.default_rng(6001).integers(0, 256, n * 4096 + rxg.TX_MAX_DATA, dtype=np.uint8)
    so = np.arange(n) * 4096 + (5 * np.arange(n) + 1) % 16
    so[I_MAX] = n * 4096 + 4                                # behind the others' bytes
    payload[so[I_MAX]:so[I_MAX] + dl[I_MAX]] = 0xFF
    segs = ref.make_segs(dl, so, 8, seed=6002)
    segs["reserved"] = 1 + np.arange(n)
    m = I_MAX
    segs["flow"][m], segs["seq"][m], segs["ack"][m], segs["win_raw"][m] = 8, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF
    segs["ip_id"][m], segs["tcp_flags"][m] = 0xFFFF, 0xFF
    off, nslots = ref.packed_offsets(dl + ol)
    carry_at = int(so[I_CARRY]) + 700                       # payload byte 700: frame offset 66 + 700, even
    for i, (_, O, w) in enumerate(ZERO_TCP):
        opts[i]["bytes"][w - HDR:w - HDR + 2] = 0
    segs["ip_id"][I_IP] = 0
    payload[carry_at:carry_at + 2] = 0
    case = Case(payload, flows, segs, opts, off, nslots, labels=dict(O=ol))
    pool, flen, _ = case.model()
    for i, (_, O, w) in enumerate(ZERO_TCP):
        a = int(off[i]) * 64
        opts[i]["bytes"][w - HDR:w - HDR + 2] = pool[a + 50:a + 52]
    a = int(off[I_IP]) * 64
    segs["ip_id"][I_IP] = int(pool[a + 24]) | int(pool[a + 25]) << 8  # stored without a byte swap
    a = int(off[I_CARRY]) * 64
    s0 = tcp_sum32(pool[a:], int(flen[I_CARRY]))
    w = (0xFFFF - (s0 & 0xFFFF)) & 0xFFFF                  # the sum's low half 0xFFFF under a high half >= 1
    payload[carry_at], payload[carry_at + 1] = w & 0xFF, w >> 8
    return case


def peer_tcbs(flows):
    """The peers' TCBs for our flows: our segment's dst_port / dst_addr are theirs."""
    t = np.zeros(len(flows), dtype=rxg.TCB_DTYPE)
    t["dport"], t["sport"] = flows["sport"], flows["dport"]
    t["ipv4_dst"] = flows["ipv4_src"].byteswap()
    t["ipv4_src"] = flows["ipv4_dst"].byteswap()
    t["state"] = rxg.TCP_ESTABLISHED
    t["identifier"] = 1 + np.arange(len(flows))
    return t
