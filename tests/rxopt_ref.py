"""The received-option rule of include/rxg.h (rxg_rx_opt) restated in plain Python, from the
rule's text: the model the GPU output (rxg_rx_opts_dev) and the host parser (rxg_rx_opt_parse)
are compared with.  It works on a frame as a list of byte values that reads zero at and beyond
the frame's length, and walks the option bytes one TLV at a time."""
import numpy as np

import rxg

CANDIDATE_VERDICTS = (rxg.V_DISPATCH, rxg.V_RST_NOPCB, rxg.V_RST_LISTEN_NONSYN)
ZERO = dict(tsval=0, tsecr=0, mss=0, wscale=0, nsack=0, sack_off=0, opt_len=0, flags=0)
FIELDS = ("tsval", "tsecr", "mss", "wscale", "nsack", "sack_off", "opt_len", "flags")


def parse(frame: bytes) -> dict:
    """The record of one frame taken as a TCP segment."""
    n = len(frame)

    def at(i):
        return frame[i] if i < n else 0

    rec = dict(ZERO)
    flags = rxg.O_PARSED
    d = at(46) >> 4
    if d < 5:
        size = 0
        flags |= rxg.O_BAD_DOFF
    else:
        size = 4 * d - 20
    if 54 + size > n:
        flags |= rxg.O_CUT
    b = [at(54 + j) for j in range(size)]
    p = 0
    while p < size:
        kind = b[p]
        if kind == 0:
            break
        if kind == 1:
            p += 1
            continue
        if p + 1 >= size:
            flags |= rxg.O_MALFORMED
            break
        length = b[p + 1]
        if length < 2 or p + length > size:
            flags |= rxg.O_MALFORMED
            break
        value = b[p + 2:p + length]
        if kind == 2 and length == 4:
            rec["mss"] = int.from_bytes(bytes(value), "big")
            flags |= rxg.O_MSS
        elif kind == 3 and length == 3:
            rec["wscale"] = value[0]
            flags |= rxg.O_WSCALE
        elif kind == 4 and length == 2:
            flags |= rxg.O_SACK_PERM
        elif kind == 5 and length in (10, 18, 26, 34):
            rec["nsack"] = (length - 2) // 8
            rec["sack_off"] = 54 + p + 2
            flags |= rxg.O_SACK
        elif kind == 8 and length == 10:
            rec["tsval"] = int.from_bytes(bytes(value[:4]), "big")
            rec["tsecr"] = int.from_bytes(bytes(value[4:]), "big")
            flags |= rxg.O_TS
        else:
            flags |= rxg.O_OTHER
        p += length
    rec["opt_len"] = size
    rec["flags"] = flags
    return rec


def as_tuple(rec) -> tuple:
    return tuple(int(rec[f]) for f in FIELDS)


def records(frames, verdicts) -> np.ndarray:
    """What rxg_rx_opts_dev writes for a burst: the parse of every candidate, zeros elsewhere."""
    out = np.zeros(len(frames), dtype=rxg.RX_OPT_DTYPE)
    for i, (f, v) in enumerate(zip(frames, verdicts)):
        if int(v) in CANDIDATE_VERDICTS:
            out[i] = as_tuple(parse(f))
    return out
