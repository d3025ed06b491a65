"""Reference model of rxg_tx_build_dev: a numpy restatement of what the reference does to send
one TCP segment,

  sendtcpdata  tcp_ip_stack/tcp_out.c:157-207   payload copy (add_tcp_data), the TCP header
  ip_out       tcp_ip_stack/ip.c:86-118         the IPv4 header, both checksums
  ether_out    tcp_ip_stack/etherout.c:87-99    the Ethernet header

with the two checksums computed by the oracle (oracle.tx_batch, ip.c:107-118), not here: the
model writes headers and payload with zeroed checksum fields only.  rxg's own definitions:
tos and fragment_offset are 0 (the reference leaves them as the fresh mbuf held them), and
the bytes from 54 + data_len to the next 64-byte boundary are 0.
"""
import numpy as np

import oracle
import rxg

HDR = 54


def skipped(segs, nflows, payload_bytes):
    """The descriptors rxg_tx_build_dev skips (include/rxg.h)."""
    s = segs["src_off"].astype(object)
    return (segs["flow"] >= nflows) | (segs["data_len"] > rxg.TX_MAX_DATA) | \
        np.array([int(o) + int(n) > payload_bytes for o, n in zip(s, segs["data_len"])], dtype=bool)


def frame_unsummed(flow, seg, payload) -> bytearray:
    """One segment's frame, padded with zeros to its last 64-byte line, checksum fields 0."""
    L = int(seg["data_len"])
    f = bytearray((HDR + L + 63) // 64 * 64)
    # etherout.c:87-99: ether_type htons(0x0800), d_addr = dst_mac, s_addr
    f[0:6] = bytes(flow["dst_mac"])
    f[6:12] = bytes(flow["src_mac"])
    f[12:14] = (0x0800).to_bytes(2, "big")
    # ip.c:97-106
    f[14] = 4 << 4 | 5                                             # version_ihl (ip.c:100)
    f[16:18] = (20 + 20 + L).to_bytes(2, "big")                    # total_length htons (ip.c:105)
    f[18:20] = int(seg["ip_id"]).to_bytes(2, "little")             # packet_id = count++, no swap (ip.c:106)
    f[22] = 127                                                    # time_to_live (ip.c:103)
    f[23] = 6                                                      # next_proto_id (ip.c:101)
    f[26:30] = int(flow["ipv4_dst"]).to_bytes(4, "little")         # src_addr = ptcb->ipv4_dst (ip.c:97)
    f[30:34] = int(flow["ipv4_src"]).to_bytes(4, "big")            # dst_addr = htonl(ipv4_src) (ip.c:99)
    # tcp_out.c:174-193
    f[34:36] = int(flow["dport"]).to_bytes(2, "big")               # src_port = htons(dport) (:174)
    f[36:38] = int(flow["sport"]).to_bytes(2, "big")               # dst_port = htons(sport) (:175)
    f[38:42] = int(seg["seq"]).to_bytes(4, "big")                  # sent_seq = htonl(next_seq) (:176)
    f[42:46] = int(seg["ack"]).to_bytes(4, "big")                  # recv_ack = htonl(ack) (:187)
    f[46] = 0x50                                                   # data_off: 20 bytes (:160-167,188)
    f[47] = int(seg["tcp_flags"])                                  # (:189)
    f[48:50] = int(seg["win_raw"]).to_bytes(2, "little")           # rx_win = 0xffff, no swap (:190)
    # cksum 0 (:191), tcp_urp 0 (:192); add_tcp_data (:158): the payload after the header
    o = int(seg["src_off"])
    f[HDR:HDR + L] = bytes(payload[o:o + L])
    return f


def build(payload, flows, segs, off64, nslots, fill=0):
    """The frame pool after rxg_tx_build_dev over a pool of nslots slots holding `fill`:
    (pool u8, len u16, stats u64[2])."""
    n = len(segs)
    skip = skipped(segs, len(flows), len(payload))
    pool = np.full(nslots * 64, fill, dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    idx = [i for i in range(n) if not skip[i]]
    for i in idx:
        f = frame_unsummed(flows[int(segs[i]["flow"])], segs[i], payload)
        pool[int(off64[i]) * 64:int(off64[i]) * 64 + len(f)] = np.frombuffer(bytes(f), np.uint8)
        lens[i] = HDR + int(segs[i]["data_len"])
    if idx:  # ip.c:107 hdr_checksum, ip.c:109-118 tcp cksum, by the oracle
        sel = np.array(idx)
        pool = oracle.tx_batch(pool, np.asarray(off64, dtype=np.uint32)[sel], lens[sel])
    return pool, lens, np.array([len(idx), n - len(idx)], dtype=np.uint64)


# -------------------------------------------------------------------- test inputs ---
LENGTHS = [0, 1, 2, 9, 10, 11, 15, 16, 17, 63, 64, 65, 73, 74, 75, 999, 1000, 1459, 1460, 1461, 8960, 65481]


def lanes_per_frame(L):
    """The size class of a segment of data_len L, named by its lanes per frame, from the rule
    in rxg_txbuild.hip's header comment: a frame of ceil((54 + L) / 64) lines; one line: class
    0 (the one-line path), up to 4 / 8 / 16 / 32 lines: 4 / 8 / 16 / 32 lanes, more: 64."""
    lines = -(-(HDR + int(L)) // 64)
    for most, lanes in ((1, 0), (4, 4), (8, 8), (16, 16), (32, 32)):
        if lines <= most:
            return lanes
    return 64


def chunks_of(L):
    """NC: the frame's 16-byte chunks, four per line."""
    return 4 * -(-(HDR + int(L)) // 64)


CLASSES = [0, 4, 8, 16, 32, 64]
# class -> (smallest, largest) data_len, by the same rule: k lines hold 64 k - 54 payload bytes
CLASS_RANGE = {0: (0, 10), 4: (11, 4 * 64 - HDR), 8: (4 * 64 - HDR + 1, 8 * 64 - HDR),
               16: (8 * 64 - HDR + 1, 16 * 64 - HDR), 32: (16 * 64 - HDR + 1, 32 * 64 - HDR),
               64: (32 * 64 - HDR + 1, rxg.TX_MAX_DATA)}
# both ends of every class (class 64: its lower end), one odd length inside each streamed
# class whose last round is partial where the class has one (139: NC 16 = 4 rounds of 4;
# 331: NC 28; 715: NC 52; 1483: NC 100), and 2731 (NC 176), a class-64 length of 44 lines
CLASS_LENGTHS = [0, 10, 11, 202, 203, 458, 459, 970, 971, 1994, 1995, 139, 331, 715, 1483, 2731]


def make_flows(n=8, seed=7):
    """n flows with distinct MACs, addresses and ports."""
    r = np.random.default_rng(seed)
    fl = np.zeros(n, dtype=rxg.TX_FLOW_DTYPE)
    fl["dport"] = 80 + np.arange(n) * 101
    fl["sport"] = 40000 + np.arange(n) * 257
    fl["ipv4_dst"] = [rxg.ip_raw(10, 1, k, 2 + k) for k in range(n)]
    fl["ipv4_src"] = [rxg.ip_host(192, 168, 3 + k, 9 + 2 * k) for k in range(n)]
    fl["dst_mac"] = r.integers(0, 256, (n, 6), dtype=np.uint8)
    fl["src_mac"] = np.frombuffer(rxg.REF_SRC_MAC, np.uint8)
    fl["src_mac"][1:, 5] += np.arange(1, n, dtype=np.uint8)
    return fl


def make_segs(lens, src_offs, nflows, seed):
    r = np.random.default_rng(seed)
    n = len(lens)
    s = np.zeros(n, dtype=rxg.TX_SEG_DTYPE)
    s["src_off"] = src_offs
    s["data_len"] = lens
    s["flow"] = r.integers(0, nflows, n)
    s["seq"] = r.integers(0, 1 << 32, n, dtype=np.uint64)
    s["ack"] = r.integers(0, 1 << 32, n, dtype=np.uint64)
    s["win_raw"] = r.integers(0, 1 << 16, n)
    s["ip_id"] = r.integers(0, 1 << 16, n)
    s["tcp_flags"] = r.integers(0, 256, n)
    return s


def slots_of(lens):
    return (HDR + np.asarray(lens, dtype=np.int64) + 63) // 64


def packed_offsets(lens, perm=None):
    """Slots for frames of these payload lengths laid out back to back in the order `perm`
    (default: as given).  Returns (off64 u32, total slots)."""
    sl = slots_of(lens)
    order = np.arange(len(sl)) if perm is None else np.asarray(perm)
    off = np.zeros(len(sl), dtype=np.uint32)
    off[order] = np.concatenate([[0], np.cumsum(sl[order])[:-1]]).astype(np.uint32)
    return off, int(sl.sum())
