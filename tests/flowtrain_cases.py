"""Case sets for the flow-train tests (tests/test_flowtrain_host.py, tests/test_gpu_flowtrain.py):
crafted records in the three layouts with every bit outside the decoded fields random, the frames
that carry their seq, and the claims each set makes about where its edges fall (asserted on the
set itself in test_flowtrain_host.py)."""
from dataclasses import dataclass, field

import numpy as np

import flowsum_cases as fc
import rxg

TILE = rxg.FLOW_TRAIN_TILE              # pairs per tile of the sort and of the cut
ROUND = rxg.FLOW_TRAIN_ROUND_LANES      # lanes a workgroup takes a tile with, per round
SCAN = rxg.FLOW_TRAIN_SCAN_ROUND        # entries per round of a one-workgroup scan
SELECT_SCAN_FRAMES = SCAN * 64          # frames whose slice counts fill one round of the select's scan
SORT_SCAN_FRAMES = SCAN // 256 * TILE   # frames whose tiles' digit counts fill one round of a pass's scan
ACK, FIN, SYN = 0x10, 0x01, 0x02
OK = fc.OK


def passes_needed(ntcb):
    """The 8-bit passes a sort on tcb_idx < ntcb needs: as many as ntcb - 1 has bytes (at least 1).
    What a set claims about itself; the kernel's own count is not observable (an extra pass over
    a digit that is zero everywhere changes no byte)."""
    return max(1, (max(ntcb - 1, 1).bit_length() + 7) // 8)


@dataclass
class Case:
    name: str
    rec48: np.ndarray                   # the fields the rule decodes (flowsum_cases.craft)
    ntcb: int
    flags: int = 0
    cur_seq: object = None              # {tcb: value} (others 0), or None for NULL
    lens: object = 54                   # frame lengths (REC8 / REC16)
    claims: dict = field(default_factory=dict)

    @property
    def n(self):
        return len(self.rec48)

    def cur_array(self):
        if self.cur_seq is None:
            return None
        a = np.zeros(self.ntcb, np.uint32)
        for k, v in self.cur_seq.items():
            a[k] = v
        return a

    def records(self, rec_kind, seed=0):
        """The records as a burst of that kind would hold them (uint8), every bit the rule does not
        decode random: checksums, state, the TCP flags but FIN, the record flags but TCP_OK, the
        tuple and ack of rxg_rec48, the spare bits of rxg_rec8."""
        rng = np.random.default_rng(seed + 7 * rec_kind)
        n = self.n
        r = self.rec48.copy()
        c = r["c"]
        c["ip_cksum"], c["tcp_cksum"] = rng.integers(0, 1 << 16, n), rng.integers(0, 1 << 16, n)
        c["state"] = rng.integers(0, 7, n)
        c["tcp_flags"] = (c["tcp_flags"] & FIN) | (rng.integers(0, 256, n).astype(np.uint8) & ~np.uint8(FIN))
        c["flags"] = (c["flags"] & rxg.F_TCP_OK) | (rng.integers(0, 64, n).astype(np.uint8) & ~np.uint8(rxg.F_TCP_OK))
        r["c"] = c
        for f in ("ether_type", "sport", "dport", "l4_proto", "version_ihl", "ack", "src_ip", "dst_ip_raw", "data_off",
                  "reserved"):
            r[f] = rng.integers(0, 1 << (8 * r.dtype[f].itemsize), n, dtype=np.uint64)
        if rec_kind == rxg.REC8:
            r8 = rxg.rec8_pack(np.ascontiguousarray(r["c"]))
            r8["w0"] |= rng.integers(0, 4, n).astype(np.uint32) << 30
            r8["w1"] |= rng.integers(0, 2, n).astype(np.uint32) << 31
            return np.ascontiguousarray(r8).view(np.uint8)
        return np.ascontiguousarray(fc.as_kind(r, rec_kind)).view(np.uint8)

    def frames(self, fill=0xEE):
        return fc.frames_for(self.rec48, self.lens, fill)


def craft(tcb, seq, datalen, tcp_flags=ACK, flags=OK, verdict=rxg.V_DISPATCH):
    return fc.craft(tcb, seq=np.asarray(seq, np.int64) & 0xFFFFFFFF, datalen=datalen, tcp_flags=tcp_flags, flags=flags,
                    verdict=verdict)


def runs(tcb, seed=0, p_cont=0.8, p_fin=0.02, datalen=None):
    """Segments of the flows tcb[i] in that packet order: each continues its flow's previous one
    with probability p_cont, else starts anywhere."""
    rng = np.random.default_rng(seed)
    tcb = np.asarray(tcb, np.int64)
    n = len(tcb)
    dl = rng.integers(1, 1461, n) if datalen is None else np.broadcast_to(datalen, (n,)).astype(np.int64)
    jump = rng.random(n) >= p_cont
    rnd = rng.integers(1, 1 << 32, n)
    seq = np.zeros(n, np.int64)
    nxt = {}
    for i, t in enumerate(tcb.tolist()):
        seq[i] = rnd[i] if (jump[i] or t not in nxt) else nxt[t]
        nxt[t] = (seq[i] + dl[i]) & 0xFFFFFFFF
    fl = np.where(rng.random(n) < p_fin, ACK | FIN, ACK)
    return craft(tcb, seq, dl, fl)


# ------------------------------------------------------------------------- select ---
def mixed(n, ntcb=37, seed=0):
    """Every verdict, index, length and checksum-flag edge of the selection, at random."""
    rng = np.random.default_rng(seed)
    r = runs(rng.integers(0, ntcb, n), seed)
    c = r["c"]
    c["verdict"] = np.where(rng.random(n) < 0.7, rxg.V_DISPATCH, rng.integers(1, 6, n))
    edge = rng.random(n) < 0.25
    c["datalen"] = np.where(edge, rng.choice([-3, 0, 1, 65535, 65536], n), c["datalen"])
    c["tcb_idx"] = np.where(rng.random(n) < 0.1, rng.choice([-1, ntcb - 1, ntcb], n), c["tcb_idx"])
    c["flags"] = np.where(rng.random(n) < 0.2, rxg.F_IP_OK, OK)
    r["c"] = c
    return r


SIZES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def select_cases():
    out = []
    for n in SIZES:
        out.append(Case(f"mixed, {n} frames", mixed(n, seed=n), 37, claims={"n": n}))
        out.append(Case(f"mixed, {n} frames, TCP_OK only", mixed(n, seed=n + 1), 37, flags=rxg.FT_TCP_OK_ONLY,
                        claims={"n": n, "left_out": n >= 63}))
        out.append(Case(f"all segments, {n} frames", runs(np.arange(n) % 5, n), 5, claims={"n": n, "S": n}))
    for lane in (0, 31, 32, 63):
        n = 4 * 64
        r = runs(np.arange(n) % 3, lane)
        c = r["c"]
        c["verdict"] = np.where(np.arange(n) % 64 == lane, rxg.V_DISPATCH, rxg.V_DROP_NONTCP)
        r["c"] = c
        out.append(Case(f"segments on lane {lane} only", r, 3, claims={"S": 4, "lanes": [lane]}))
    r = runs(np.arange(300) % 4, 1)
    c = r["c"]
    c["verdict"] = rxg.V_ARP
    r["c"] = c
    out.append(Case("no segments", r, 4, claims={"S": 0}))
    r = runs(np.arange(130) % 4, 2)
    c = r["c"]
    c["verdict"] = np.where(np.arange(130) == 129, rxg.V_DISPATCH, rxg.V_DROP_L2)
    r["c"] = c
    out.append(Case("a partial last slice whose last frame is the only segment", r, 4,
                    claims={"S": 1, "n": 130, "lanes": [1]}))
    # each field edge on its own, one frame each, in flow 2 of 3 (tcb_idx ntcb - 1)
    tcb = [-1, 2, 3, 2, 2, 2, 2, 2] + [2] * 6
    dl = [10, 10, 10, -3, 0, 1, 65535, 65536] + [10] * 6
    vd = [0] * 8 + [0, 1, 2, 3, 4, 5]
    out.append(Case("field edges one by one", craft(tcb, np.arange(14) * 100000 + 5, dl, verdict=np.array(vd)), 3,
                    claims={"S": 4, "out": 2}))
    return out


# --------------------------------------------------------------------------- sort ---
NTCBS = [1, 255, 256, 257, 65535, 65536, 65537, 1 << 24]


def digit_flows(ntcb):
    """Index 0, ntcb - 1, and the digit values 0x00 and 0xFF of every pass."""
    want = {0, ntcb - 1, 0xFF, 0x100, 0xFF00, 0xFFFF, 0x10000, 0xFF0000, 0xFF00FF, 0xFFFF00, 0xFFFFFE, 0x1FF, 0x100FF}
    return sorted(t for t in want if 0 <= t < ntcb and t <= fc.REC8_MAX_TCB)


def sort_cases():
    out = []
    for ntcb in NTCBS:
        flows = np.array(digit_flows(ntcb))
        rng = np.random.default_rng(ntcb)
        out.append(Case(f"ntcb {ntcb}: flows at 0, the top and the digit edges", runs(rng.choice(flows, 200), ntcb), ntcb,
                        claims={"passes": passes_needed(ntcb), "flows": len(flows)}))
    out.append(Case("300 segments of one flow", runs(np.full(300, 6), 1, p_cont=0.5), 9, claims={"S": 300}))
    out.append(Case("a tile plus one, all of one flow", runs(np.full(TILE + 1, 0), 2, p_cont=0.9), 1,
                    claims={"S": TILE + 1}))
    out.append(Case("1 025 flows in descending order", runs(np.arange(1025)[::-1].copy(), 3), 1025,
                    claims={"S": 1025, "passes": 2}))
    out.append(Case("two flows alternating", runs(np.tile([250, 3], 100), 4, p_cont=0.9), 251, claims={"S": 200}))
    top = np.random.default_rng(5).permutation(np.repeat(np.arange(6) << 16, 50))
    out.append(Case("flows that differ only in the top digit", runs(top, 5), (5 << 16) + 1,
                    claims={"passes": 3, "S": 300}))
    both = np.concatenate([np.full(TILE, 7 + 256 * 3), np.random.default_rng(6).permutation(TILE) % 256])
    out.append(Case("a one-digit tile beside a 256-digit tile", runs(both, 6), 1024, claims={"S": 2 * TILE, "passes": 2}))
    return out


# ---------------------------------------------------------------------------- cut ---
def chain(tcb, seq0, lens, fl=None):
    """Contiguous segments of one flow from seq0."""
    lens = np.asarray(lens, np.int64)
    seq = seq0 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    return craft(np.full(len(lens), tcb), seq, lens, ACK if fl is None else np.asarray(fl))


def cat(*parts):
    return np.concatenate(parts)


def cut_cases():
    out = []
    for k in (1, 2, 63, 64, 65, TILE + 1):
        out.append(Case(f"a train of {k}", cat(chain(1, 999, [7]), chain(2, 5000, [100] * k), chain(2, 77, [3])), 4,
                        cur_seq={2: 5000}, claims={"T": 3, "nseg": k}))
    # the sorted list is flow 0's 60 (or TILE - 3) single segments, then flow 1's train
    for lead, what in ((60, "wave"), (TILE - 3, "tile")):
        singles = craft(np.zeros(lead), np.arange(lead) * 3000 + 1, 5)
        out.append(Case(f"a train across a {what} edge of the sorted list", cat(chain(1, 10, [9] * 8), singles), 2,
                        claims={"T": lead + 1, "span": (lead, lead + 8)}))
    out.append(Case("contiguous across two flows: no join", cat(chain(3, 100, [50, 50]), chain(4, 200, [50])), 5,
                    claims={"T": 2}))
    out.append(Case("two other flows' frames between contiguous segments: join",
                    cat(chain(3, 100, [50]), chain(1, 150, [1]), chain(5, 150, [1]), chain(3, 150, [50])), 6,
                    claims={"T": 3}))
    out.append(Case("gap, overlap, duplicate", craft([1] * 7, [100, 151, 201, 250, 300, 300, 350], 50), 2,
                    claims={"T": 4}))
    out.append(Case("FIN in the middle and at the end",
                    chain(1, 100, [10] * 5, [ACK, ACK | FIN, ACK, ACK, ACK | FIN]), 2, cur_seq={1: 100},
                    claims={"T": 2, "fins": 2}))
    out.append(Case("SYN on a data segment", chain(1, 100, [10] * 3, [ACK, ACK | SYN, ACK]), 2, claims={"T": 1}))
    out.append(Case("a wrapping segment between two it would connect",
                    chain(1, 0xFFFFFFF0 - 10, [10, 0x20, 10]), 2, cur_seq={1: 0xFFFFFFF0 - 10},
                    claims={"T": 3, "wraps": 1}))
    out.append(Case("a segment ending exactly at 2^32 wraps", chain(1, 0xFFFFFFF0 - 10, [10, 0x10, 10]), 2,
                    cur_seq={1: 0xFFFFFFF0 - 10}, claims={"T": 3, "wraps": 1}))
    out.append(Case("a train ending at 0xFFFFFFFF, then a segment at 0",
                    cat(chain(1, 0xFFFFFFFF - 30, [10, 20]), chain(1, 0, [5])), 2, cur_seq={1: 0xFFFFFFFF - 30},
                    claims={"T": 2, "wraps": 0, "heads": 1}))
    heads = cat(chain(0, 500, [5, 5]), chain(1, 500, [5]), chain(2, 0, [5]), chain(3, 40, [5]), chain(3, 900, [5]),
                chain(4, 0xFFFFFFFE, [9]))
    out.append(Case("cur_seq NULL", heads, 5, claims={"heads": 0}))
    out.append(Case("cur_seq equal, off by one, 0 with seq 0, a second train's, a wrapping segment's", heads, 5,
                    cur_seq={0: 500, 1: 501, 2: 0, 3: 900, 4: 0xFFFFFFFE}, claims={"heads": 1}))
    for ln in (38, 39, 40, 41, 42, 54):
        out.append(Case(f"frames cut at {ln} bytes", chain(1, 0xA1B2C3D4, [6, 6, 6]), 2, lens=ln,
                        cur_seq={1: 0xA1B2C3D4 if ln >= 42 else 0xA1B2C3D4 & ~((1 << (8 * (42 - ln))) - 1) if ln > 38 else 0},
                        claims={"truncated": ln < 42}))
    return out


def rule_cases():
    """Every set at its CPU size."""
    return select_cases() + sort_cases() + cut_cases()


# ---------------------------------------------------------------- scan edges (GPU) ---
def big(n, nflows=1000, run=64, seed=0):
    """n frames, all segments: flows arriving in runs of `run` contiguous segments."""
    rng = np.random.default_rng(seed)
    nruns = (n + run - 1) // run
    tcb = np.repeat(rng.integers(0, nflows, nruns), run)[:n]
    dl = 1448
    # a flow's runs follow each other in sequence space with probability 1/2
    start = rng.integers(1, 1 << 31, nruns)
    seq = (np.repeat(start, run)[:n] + (np.arange(n) % run) * dl) & 0xFFFFFFFF
    return craft(tcb, seq, dl)


SCAN_SIZES = [SORT_SCAN_FRAMES - TILE, SORT_SCAN_FRAMES, SORT_SCAN_FRAMES + 1, SELECT_SCAN_FRAMES - 64,
              SELECT_SCAN_FRAMES, SELECT_SCAN_FRAMES + 1]
