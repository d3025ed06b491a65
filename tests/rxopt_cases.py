"""Deterministic frame sets for the received-option parse (rxg_rx_opts_dev, rxg_rx_opt_parse):
every set is a list of frames; SETS names them all.  The frames go to the table of table():
an established flow (the default source), a listener on :80 and a closed port, so the three
candidate verdicts occur.  poisoned_arena() packs a set like pktgen.pack_arena but fills what
follows each frame's last byte, up to its line's end, with bytes that parse as valid options:
a read at or beyond len, or into a neighbour's slot, shows up in the record."""
import random
import struct

import numpy as np

import pktgen

DST = pktgen.ip4(192, 168, 78, 2)
NOP, EOL = b"\x01", b"\x00"
ALIGNED_TS = bytes([1, 1, 8, 10])
CUT_LENS = [54, 55, 63, 64, 65, 79, 80, 81, 93, 94, 95, 200]
GENERAL_LANES = [0, 1, 31, 32, 33, 62, 63]
SIZES = [0, 1, 63, 64, 65, 257]
# what a byte past a frame's end holds, by its offset from frame byte 54: a timestamp, an MSS
# and two no-operations (16 bytes, so the phase is the same in every line)
POISON = bytes([8, 10, 0xDE, 0xAD, 0xBE, 0xEF, 0xFE, 0xED, 0xFA, 0xCE, 2, 4, 0x7A, 0x69, 1, 1])


def table():
    rows = [(80, 0, pktgen.raw_of_host(DST), 0, pktgen.LISTENING),
            (80, 1024, pktgen.raw_of_host(DST), pktgen.ip4(10, 0, 0, 1), pktgen.ESTABLISHED)]
    return pktgen.table_arrays(rows)


def seg(opts: bytes = b"", payload: bytes = b"", **kw) -> bytes:
    """A segment of the established flow whose header carries exactly `opts` (a multiple of 4)."""
    assert len(opts) % 4 == 0 and len(opts) <= 40
    return pktgen.frame(doff=5 + len(opts) // 4, tcp_opts=opts, payload=payload, **kw)


def mss(v=1460):
    return bytes([2, 4]) + struct.pack(">H", v)


def wscale(v=7):
    return bytes([3, 3, v])


def sack_perm():
    return bytes([4, 2])


def sack(nblocks, base=0x1000):
    return bytes([5, 2 + 8 * nblocks]) + b"".join(struct.pack(">II", base + 16 * k, base + 16 * k + 8)
                                                   for k in range(nblocks))


def timestamp(tsval, tsecr):
    return bytes([8, 10]) + struct.pack(">II", tsval & 0xFFFFFFFF, tsecr & 0xFFFFFFFF)


def aligned_ts(tsval, tsecr):
    return NOP + NOP + timestamp(tsval, tsecr)


def tail(kind: str, room: int, rng) -> bytes:
    """`room` bytes after an option: end of list, no-operations, or unrelated bytes (an unknown
    kind that takes the room when it can carry a length byte)."""
    if kind == "eol":
        return EOL * room
    if kind == "nop" or room < 2:
        return NOP * room
    return bytes([rng.choice([9, 30, 254]), room]) + rng.randbytes(room - 2)


def placement():
    rng = random.Random(11)
    out = []
    for size in range(0, 44, 4):
        if size == 0:
            out.append(seg())
        for make in (lambda k: mss(1000 + k), lambda k: wscale(k % 15), lambda k: sack_perm(), lambda k: sack(1, k << 8),
                     lambda k: timestamp(0x01020304 * (k + 1), 0xA0B0C0D0 + k)):
            for p in range(size):
                opt = make(size + p)
                if p + len(opt) > size:
                    break
                for t in ("eol", "nop", "other"):
                    out.append(seg(NOP * p + opt + tail(t, size - p - len(opt), rng), payload=rng.randbytes(rng.randrange(0, 9))))
    return out


KNOWN = {2: 4, 3: 3, 4: 2, 5: 10, 8: 10}


def boundaries():
    rng = random.Random(12)
    out = []
    for size in (4, 12, 40):
        for kind, ln in KNOWN.items():
            if ln > size:
                continue
            body = rng.randbytes(ln - 2)
            out.append(seg(NOP * (size - ln) + bytes([kind, ln]) + body))                 # ends exactly at O
            out.append(seg((NOP * (size - ln + 1) + bytes([kind, ln]) + body)[:size]))    # one byte past O
            out.append(seg(NOP * (size - ln) + bytes([kind, ln + 1]) + body))             # claims one byte past O
        for bad in (0, 1):
            for kind in (2, 8, 77):
                out.append(seg(bytes([kind, bad]) + mss()[:2] + NOP * (size - 4)))        # length byte 0 / 1 at the start
                lead = mss(900 + bad) + NOP * (size - 6) if size >= 8 else NOP * 2
                out.append(seg(lead + bytes([kind, bad])))                                # and in the last two bytes
        for kind in (2, 5, 8, 200):
            out.append(seg(NOP * (size - 1) + bytes([kind])))                             # no length byte
    for kind in KNOWN:                                                                    # every wrong length
        for ln in range(2, 41):
            if ln == KNOWN[kind] or (kind == 5 and ln in (10, 18, 26, 34)):
                continue
            out.append(seg((bytes([kind, ln]) + rng.randbytes(ln - 2) + mss(ln) + EOL * 40)[:40]))
    return out


def repeats():
    return [seg(timestamp(1, 2) + timestamp(3, 4)), seg(aligned_ts(5, 6) + aligned_ts(7, 8)),
            seg(sack(1) + sack(2) + NOP * 2 + NOP * 8 + NOP * 2), seg(sack(2, 0x100) + sack(1, 0x200) + NOP * 12),
            seg(mss(100) + mss(200)), seg(wscale(1) + wscale(14) + NOP * 2), seg(mss(536) + timestamp(9, 9) + mss(1200) + NOP * 2)]


def sacks():
    out = []
    for nb in (1, 2, 3, 4):
        ln = 2 + 8 * nb
        out.append(seg(sack(nb) + NOP * (40 - ln)))       # sack_off 56, the lowest
        out.append(seg(NOP * (40 - ln) + sack(nb)))       # the highest for this many blocks
        mid = NOP * 2 + sack(nb)
        out.append(seg(mid + NOP * (-len(mid) % 4)))      # behind two no-operations, as peers send it
    out.append(seg(NOP * 30 + sack(1)))                   # sack_off 86, the highest of all
    return out


def data_offs():
    body = aligned_ts(0x11111111, 0x22222222) + mss() + sack_perm() + wscale(3) + NOP * 19
    assert len(body) == 40
    return [pktgen.frame(doff=d, tcp_opts=b"", payload=body + b"payload") for d in range(16)]


def cut_frames():
    """data_off 15 and every cut length; whole, the 40 bytes hold options all the way.  The last
    frame is a 60-byte one: the pool ends at its line."""
    body = timestamp(0x0A0B0C0D, 0x01020304) + mss(1400) + sack(1) + wscale(9) + sack_perm() + timestamp(5, 6) + NOP
    assert len(body) == 40
    whole = seg(body, payload=bytes(range(120)))
    out = [whole[:n] for n in CUT_LENS for _ in (0, 1)]
    out += [seg(aligned_ts(3, 4), payload=b"x" * 40)[:n] for n in (58, 62, 66, 70)]
    out.append(whole[:60])
    return out


def zero_records():
    rng = random.Random(13)
    out = [pktgen.frame(proto=17, doff=15, tcp_opts=aligned_ts(1, 2) + NOP * 28),
           pktgen.frame(proto=1, payload=rng.randbytes(60)),
           b"\xff" * 6 + rng.randbytes(6) + b"\x08\x06" + rng.randbytes(28) + aligned_ts(1, 2) * 4,
           rng.randbytes(12) + b"\x86\xdd" + seg(aligned_ts(1, 2))[14:],
           rng.randbytes(12) + b"\x81\x00" + rng.randbytes(80)]
    whole = seg(aligned_ts(9, 9) + mss() + NOP * 24, payload=b"tail")
    out += [whole[:n] for n in (0, 1, 13, 14, 23, 24, 34, 46, 47, 53)]
    return out


def general(k: int) -> bytes:
    """A frame that needs the walk."""
    forms = [mss(1000 + k) + sack_perm() + timestamp(k, k + 1) + NOP + wscale(k % 15),
             timestamp(k, 0) + NOP * 2, aligned_ts(k, 1) + NOP * 2 + sack(1, k), mss(k) + NOP * 4,
             NOP * 3 + bytes([8]), NOP * 28 + aligned_ts(k, 77)]
    return seg(forms[k % len(forms)], payload=b"g" * (k % 5))


def slices():
    """64-frame slices, one after another (the set starts a batch, so they are the kernel's)."""
    def al(k):
        return seg(aligned_ts(0x1000 + k, 0x2000 + k), payload=b"d" * (k % 70))
    out = [al(k) for k in range(64)]                                       # all aligned timestamps
    out += [seg(payload=b"n" * (k % 70)) for k in range(64)]               # no options
    out += [al(k) if k % 3 else seg() for k in range(64)]                  # both fast kinds
    for lane in GENERAL_LANES:                                             # one general frame
        out += [general(lane) if k == lane else al(k) for k in range(64)]
    out += [general(k) for k in range(64)]                                 # general on every lane
    out += [al(k) if k != 5 else general(k) for k in range(17)]            # a partial last slice
    return out


def general_lanes(frames):
    """Per 64-frame slice of `frames`: the lanes whose frame is neither option-less nor the aligned
    timestamp alone."""
    res = []
    for s in range(0, len(frames), 64):
        lanes = []
        for k, f in enumerate(frames[s:s + 64]):
            size = 4 * (f[46] >> 4) - 20 if len(f) > 46 else 0
            if not (size <= 0 or (size == 12 and f[54:58] == ALIGNED_TS)):
                lanes.append(k)
        res.append(lanes)
    return res


def random_tlv(seed=21, n=3000):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        size = 4 * rng.randrange(0, 11)
        b = bytearray()
        while len(b) < size:
            r = rng.random()
            if r < 0.15:
                b += NOP
            elif r < 0.20:
                b += EOL
            elif r < 0.65:
                b += rng.choice([mss(rng.getrandbits(16)), wscale(rng.getrandbits(8)), sack_perm(),
                                 sack(rng.randrange(1, 5), rng.getrandbits(24)),
                                 timestamp(rng.getrandbits(32), rng.getrandbits(32))])
            elif r < 0.80:
                ln = rng.randrange(2, 12)
                b += bytes([rng.choice([6, 7, 9, 19, 28, 30, 34, 253, 255]), ln]) + rng.randbytes(ln - 2)
            elif r < 0.90:
                b += bytes([rng.choice(list(KNOWN)), rng.randrange(0, 41)]) + rng.randbytes(rng.randrange(0, 6))
            else:
                b += rng.randbytes(rng.randrange(1, 5))
        kw = {}
        v = rng.random()
        if v < 0.10:
            kw = dict(dport=9999)                                    # findtcb NULL
        elif v < 0.20:
            kw = dict(sport=rng.randrange(2000, 60000), flags=rng.choice([0x02, 0x10]))   # the listener: SYN or not
        f = seg(bytes(b[:size]), payload=rng.randbytes(rng.choice([0, 0, 1, 7, 30, 100])), **kw)
        if rng.random() < 0.08:
            f = f[:rng.randrange(40, len(f) + 1)]
        out.append(f)
    return out


def parity(seed=31, n=3000):
    return pktgen.parity_set(seed, n)[1]


def mixed(n=257):
    r = random_tlv(seed=22, n=n)
    return [r[k] if k % 4 else seg(aligned_ts(k, k * 3)) for k in range(n)]


SETS = dict(placement=placement, boundaries=boundaries, repeats=repeats, sacks=sacks, data_offs=data_offs,
            cut_frames=cut_frames, zero_records=zero_records, slices=slices, random_tlv=random_tlv, parity=parity)


def poisoned_arena(frames):
    """pktgen.pack_arena's layout; the bytes from a frame's end to its last line's end hold POISON
    by their offset from frame byte 54.  The allocation ends with the last frame's last line."""
    arena, off, lens = pktgen.pack_arena(frames)
    for o, ln in zip(off.tolist(), lens.tolist()):
        end = (ln + 63) // 64 * 64
        x = np.arange(ln, end)
        arena[o * 64 + ln:o * 64 + end] = np.frombuffer(POISON, np.uint8)[(x - 54) % 16]
    return arena, off, lens
