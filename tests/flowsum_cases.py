"""Case builders for the per-flow summary tests (tests/test_flowsum_host.py,
tests/test_gpu_flowsum.py): crafted records, the frames that carry their seq and ack, and real
traffic on a table whose slot f holds flow f."""
import random

import numpy as np

import pktgen
import rxg

DST = pktgen.ip4(192, 168, 78, 2)
ESTABLISHED = 4
OK = rxg.F_IP_OK | rxg.F_TCP_OK
REC8_MAX_TCB = 0xFFFFFE   # rxg_rec8 carries tcb_idx + 1 in 24 bits


def craft(tcb, seq=0, ack=0, datalen=0, tcp_flags=0x10, flags=OK, verdict=rxg.V_DISPATCH, state=ESTABLISHED):
    """REC48 records with the given fields (scalars broadcast over the arrays)."""
    tcb = np.atleast_1d(np.asarray(tcb, np.int64))
    r = np.zeros(len(tcb), rxg.REC48_DTYPE)
    c = r["c"]
    c["tcb_idx"], c["datalen"], c["tcp_flags"], c["flags"] = tcb, datalen, tcp_flags, flags
    c["verdict"], c["state"] = verdict, state
    r["c"] = c
    r["seq"], r["ack"] = np.asarray(seq, np.uint32), np.asarray(ack, np.uint32)
    return r


def as_kind(rec48, rec_kind):
    """The records as the burst would have written them in that kind (a contiguous array)."""
    if rec_kind == rxg.REC48:
        return np.ascontiguousarray(rec48)
    c = np.ascontiguousarray(rec48["c"])
    return c if rec_kind == rxg.REC16 else rxg.rec8_pack(c)


def frames_for(rec48, lens=54, fill=0xEE):
    """One frame per record carrying its seq and ack at bytes 38..46 (everything else `fill`), cut
    to lens[i] bytes."""
    lens = np.broadcast_to(np.asarray(lens), (len(rec48),))
    out = []
    for r, ln in zip(rec48, lens.tolist()):
        f = bytearray([fill]) * 64
        f[38:42] = int(r["seq"]).to_bytes(4, "big")
        f[42:46] = int(r["ack"]).to_bytes(4, "big")
        out.append(bytes(f[:ln]))
    return out


def flow_src(f):
    return pktgen.ip4(10, 1 + (f >> 16), (f >> 8) & 255, f & 255)


def table(nflows, listener=True):
    """Slot f < nflows: an ESTABLISHED flow from flow_src(f):2000 to DST:80; then a listener."""
    rows = [(80, 2000, pktgen.raw_of_host(DST), flow_src(f), ESTABLISHED) for f in range(nflows)]
    if listener:
        rows.append((80, 0, pktgen.raw_of_host(DST), 0, 1))
    return rows


def flow_frame(f, seq=1, ack=1, flags=0x10, payload=b"", **kw):
    return pktgen.frame(src_ip=flow_src(f), dst_ip=DST, sport=2000, dport=80, seq=seq, ack=ack, flags=flags,
                        payload=payload, **kw)


def traffic(flow_of, seed=0, unknown=0.0, fin=0.02, data=0.3, bad_ck=0.0):
    """A frame of flow flow_of[i] per entry (-1: a client nobody knows, an RST or a SYN to the
    listener), random seq / ack / payload; `bad_ck`: share with a flipped payload or header byte."""
    rng = random.Random(seed)
    out = []
    for f in flow_of:
        if f < 0 or rng.random() < unknown:
            out.append(pktgen.frame(src_ip=pktgen.ip4(172, 16, 1, rng.randrange(200)), dst_ip=DST, sport=40000,
                                    dport=rng.choice([80, 9999]), flags=rng.choice([0x02, 0x10]),
                                    seq=rng.getrandbits(32), ack=rng.getrandbits(32)))
            continue
        fl = 0x11 if rng.random() < fin else 0x10
        pay = rng.randbytes(rng.randrange(1, 120)) if rng.random() < data else b""
        fr = flow_frame(f, rng.getrandbits(32), rng.getrandbits(32), fl, pay)
        if bad_ck and rng.random() < bad_ck:
            b = bytearray(fr)
            b[rng.randrange(46, len(b))] ^= 0x5A
            fr = bytes(b)
        out.append(fr)
    return out


def imix(n=4096, nflows=1000, seed=3):
    """64 / 576 / 1500-byte frames at 7:4:1 over nflows flows."""
    rng = random.Random(seed)
    sizes = rng.choices([64, 576, 1500], [7, 4, 1], k=n)
    return [flow_frame(rng.randrange(nflows), rng.getrandbits(32), rng.getrandbits(32), 0x10,
                       rng.randbytes(s - 54)) for s in sizes]
