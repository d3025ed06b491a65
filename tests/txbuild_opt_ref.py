"""Reference model of rxg_tx_build_opt_dev: tests/txbuild_ref.py's frame (sendtcpdata / ip_out /
ether_out restated) extended by the segment's option block, as sendtcpack extends it
(tcp_ip_stack/tcp_out.c:251-289): total_length and data_off grow by the block's length O, the
O option bytes stand at frame byte 54 and the payload at H = 54 + O.  Both checksums are the
oracle's (oracle.tx_batch sums frame[34 .. 14 + total_length) whatever the header length),
never code under test."""
import numpy as np

import oracle
import rxg
import txbuild_ref as ref

HDR = ref.HDR
OPT_LENS = [0, 4, 8, 12, 16, 28, 40]
ALL_OPT_LENS = list(range(0, 44, 4))  # every length a block may have (tests/txbuild_opt_cases.py)


def opt_len(segs, opts, nopts=None):
    """Per segment: the option bytes O of the block its `reserved` names, or -1 where the
    descriptor is skipped for its block (reserved > nopts, a len over 40 or not a multiple
    of 4)."""
    nopts = len(opts) if nopts is None else nopts
    out = np.zeros(len(segs), dtype=np.int64)
    for i, k in enumerate(segs["reserved"].tolist()):
        if k == 0:
            continue
        if k > nopts:
            out[i] = -1
            continue
        o = int(opts[k - 1]["len"])
        out[i] = o if o <= 40 and o % 4 == 0 else -1
    return out


def skipped(segs, nflows, payload_bytes, opts, nopts=None):
    """The descriptors rxg_tx_build_opt_dev skips (include/rxg.h)."""
    o = opt_len(segs, opts, nopts)
    dl = segs["data_len"].astype(np.int64)
    return ref.skipped(segs, nflows, payload_bytes) | (o < 0) | (dl > rxg.TX_MAX_DATA - np.maximum(o, 0))


def frame_unsummed(flow, seg, payload, block) -> bytearray:
    """One segment's frame with the option bytes of `block` (None: no options), padded with
    zeros to its last 64-byte line, checksum fields 0."""
    O = int(block["len"]) if block is not None else 0
    L = int(seg["data_len"])
    base = ref.frame_unsummed(flow, seg, payload)
    f = bytearray((HDR + O + L + 63) // 64 * 64)
    f[:HDR] = base[:HDR]
    f[16:18] = (20 + 20 + O + L).to_bytes(2, "big")     # total_length (ip.c:105 with tcp_len 20 + O)
    f[46] = (5 + O // 4) << 4                            # data_off (tcp_out.c:264-265,278)
    if O:
        f[HDR:HDR + O] = bytes(block["bytes"][:O])       # the options, prepended to the data
    f[HDR + O:HDR + O + L] = base[HDR:HDR + L]           # add_tcp_data's bytes after them
    return f


def build(payload, flows, segs, opts, off64, nslots, fill=0, nopts=None):
    """The frame pool after rxg_tx_build_opt_dev over a pool of nslots slots holding `fill`:
    (pool u8, len u16, stats u64[2])."""
    n = len(segs)
    skip = skipped(segs, len(flows), len(payload), opts, nopts)
    pool = np.full(nslots * 64, fill, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    idx = [i for i in range(n) if not skip[i]]
    for i in idx:
        k = int(segs[i]["reserved"])
        f = frame_unsummed(flows[int(segs[i]["flow"])], segs[i], payload, opts[k - 1] if k else None)
        pool[int(off64[i]) * 64:int(off64[i]) * 64 + len(f)] = np.frombuffer(bytes(f), np.uint8)
        lens[i] = HDR + (int(opts[k - 1]["len"]) if k else 0) + int(segs[i]["data_len"])
    if idx:
        sel = np.array(idx)
        pool = oracle.tx_batch(pool, np.asarray(off64, dtype=np.uint32)[sel], lens[sel])
    return pool, lens, np.array([len(idx), n - len(idx)], dtype=np.uint64)


# -------------------------------------------------------------------- test inputs ---
def make_opts(lens=OPT_LENS[1:], seed=5):
    """One block per length, random option bytes, and garbage in everything the call must
    ignore: bytes[] at and past len, both reserved fields."""
    r = np.random.default_rng(seed)
    o = np.frombuffer(r.integers(0, 256, 48 * len(lens), dtype=np.uint8).tobytes(), dtype=rxg.TX_OPT_DTYPE).copy()
    o["len"] = lens
    return o


def frame_lens(data_lens, olens):
    return HDR + np.asarray(olens, dtype=np.int64) + np.asarray(data_lens, dtype=np.int64)


def packed_offsets(data_lens, olens, perm=None):
    """ref.packed_offsets for frames of 54 + O + data_len bytes."""
    return ref.packed_offsets(np.asarray(data_lens, dtype=np.int64) + np.asarray(olens, dtype=np.int64), perm)


def payload_lengths(O):
    """The payload lengths of the GPU tests for a block of O bytes: 0, 1, 2; both sides of the
    one-line edge where there is one (H + L = 64 | 65: 10 - O, 11 - O); both sides of the
    line counts at which the size class changes and of 1 line (64 k - H, + 1 for k = 1, 4, 8,
    16, 32); one length per streamed class whose last round is partial (NC = 28, 52, 100,
    176 chunks: txbuild_ref.CLASS_LENGTHS' 331, 715, 1483, 2731 less O)."""
    H = HDR + O
    s = {0, 1, 2}
    if O <= 8:
        s |= {10 - O, 11 - O}
    for k in (1, 4, 8, 16, 32):
        s |= {x for x in (64 * k - H, 64 * k - H + 1) if x >= 0}
    s |= {331 - O, 715 - O, 1483 - O, 2731 - O}
    return sorted(s)
