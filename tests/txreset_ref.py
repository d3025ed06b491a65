"""Reference model of rxg_tx_reset_dev: a numpy restatement of what the reference does to
answer one offending packet with a reset,

  send_reset  tcp_ip_stack/tcp_out.c:103-146   the TCP header mirrored from the offender's
  ip_out      tcp_ip_stack/ip.c:62-132         the IPv4 header, both checksums
  ether_out   tcp_ip_stack/etherout.c:87-99    the Ethernet header

for every frame whose verdict is RST_NOPCB or RST_LISTEN_NONSYN, in packet order.  The two
checksums are computed by the oracle (oracle.tx_batch, ip.c:107-118), not here: the model
writes the headers with zeroed checksum fields only.  rxg's own definitions: tos and
fragment_offset are 0, bytes 54-63 of a reset's line are 0, bytes of the offender at and
beyond its len read as zero, and the destination MAC is the offender's source MAC.
"""
import numpy as np

import oracle
import rxg

RST_VERDICTS = (rxg.V_RST_NOPCB, rxg.V_RST_LISTEN_NONSYN)


def offender_line(arena, off64, length) -> bytes:
    """The first 64 bytes of the frame as the kernel reads them: zero at and beyond len."""
    a = int(off64) * 64
    ln = min(int(length), 64)
    return bytes(arena[a:a + ln]) + bytes(64 - ln)


def reset_unsummed(inb: bytes, ip_id: int, src_mac: bytes) -> bytearray:
    """One reset's 64-byte line for the offender line `inb`, checksum fields 0."""
    f = bytearray(64)
    f[0:6] = inb[6:12]                                   # d_addr = get_mac(dst): the offender's s_addr
    f[6:12] = bytes(src_mac)                             # etherout.c:94-99
    f[12:14] = (0x0800).to_bytes(2, "big")               # etherout.c:89
    f[14] = 4 << 4 | 5                                   # version_ihl (ip.c:100)
    f[16:18] = (20 + 20).to_bytes(2, "big")              # total_length htons(20 + tcp_len + 0) (ip.c:105)
    f[18:20] = (ip_id & 0xFFFF).to_bytes(2, "little")    # packet_id = count++, no swap (ip.c:106)
    f[22] = 127                                          # time_to_live (ip.c:103)
    f[23] = 6                                            # next_proto_id (ip.c:101)
    f[26:30] = inb[30:34]                                # src_addr = ptcb.ipv4_dst = ip_hdr->dst_addr (tcp_out.c:142, ip.c:97)
    f[30:34] = inb[26:30]                                # dst_addr = htonl(htonl(src_addr)) (tcp_out.c:143, ip.c:99)
    f[34:36] = inb[36:38]                                # src_port = t_hdr->dst_port (tcp_out.c:127)
    f[36:38] = inb[34:36]                                # dst_port = t_hdr->src_port (:128)
    f[38:42] = inb[42:46]                                # sent_seq = t_hdr->recv_ack (:129)
    # recv_ack = 0 (:130)
    f[46] = ((20 + 3) // 4) << 4                         # data_off (:117-124)
    f[47] = rxg.TCP_FLAG_RST                             # (:131)
    f[48:50] = (12000).to_bytes(2, "little")             # rx_win = 12000, no swap (:132)
    # cksum 0 (ip.c:91), tcp_urp 0 (:133)
    return f


def build(arena, off64, lens, verdicts, ip_id0, src_mac, cap):
    """(out u8[min(count, cap) * 64], idx u32[min(count, cap)], count) of rxg_tx_reset_dev."""
    sel = [i for i, v in enumerate(verdicts) if int(v) in RST_VERDICTS]
    count = len(sel)
    sel = sel[:max(0, min(count, int(cap)))]
    out = np.zeros(len(sel) * 64, dtype=np.uint8)
    for k, i in enumerate(sel):
        f = reset_unsummed(offender_line(arena, off64[i], lens[i]), ip_id0 + k, src_mac)
        out[64 * k:64 * k + 64] = np.frombuffer(bytes(f), np.uint8)
    if sel:  # ip.c:107 hdr_checksum, ip.c:109-118 the TCP checksum, by the oracle
        out = oracle.tx_batch(out, np.arange(len(sel), dtype=np.uint32), np.full(len(sel), 54, np.uint16))
    return out, np.array(sel, dtype=np.uint32), count


def one(inb: bytes, ip_id: int, src_mac: bytes = rxg.REF_SRC_MAC) -> bytes:
    """The reset for one offender line, checksums in place."""
    line = bytes(inb[:64]) + bytes(max(0, 64 - len(inb)))
    f = np.frombuffer(bytes(reset_unsummed(line, ip_id, src_mac)), np.uint8)
    return oracle.tx_batch(f, np.zeros(1, np.uint32), np.full(1, 54, np.uint16)).tobytes()
