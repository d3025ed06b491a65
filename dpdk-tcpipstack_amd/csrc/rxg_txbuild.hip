// rxg_txbuild.hip — transmit segment build on the device (rxg_tx_build_dev).
//
// What the reference does per segment on the CPU -- sendtcpdata (tcp_out.c:157-207: get a
// buffer, add_tcp_data's memcpy of the payload, the TCP header) -> ip_out (ip.c:86-118: the
// IPv4 header, both checksums) -> ether_out (etherout.c:87-99: the Ethernet header) -- in one
// pass over a batch of segment descriptors: each payload byte is loaded once from wherever the
// socket data lives, each frame line is stored once with both checksums in place.
//
// A wave takes the launch's 64-descriptor slices wave, wave + nwaves, ...: lane i validates
// descriptor i of the slice (a skipped descriptor's flow index and source offset are never
// used as addresses), loads its flow record and writes len[i].  The slice's segments are
// then built by size class, as rx_kernel's frames are (rxg_rx_frames.h run_class): a group
// of LPF lanes per frame, 64 / LPF frames per round.
//
//   frame chunk c = frame bytes [16c, 16c + 16); a frame of data_len L has NC = 4 *
//   ceil((54 + L) / 64) of them; chunk c >= 3 holds payload bytes [16c - 54, 16c - 38)
//
//   NC == 4 (L <= 10: pure ACKs, SYN, FIN)   4 lanes per frame, 16 frames per round: lane c
//           writes chunk c; lane 3 loads the payload's one or two chunks itself
//   NC <= 16 / 32 / 64 / 128 / more          4 / 8 / 16 / 32 / 64 lanes per frame; round r
//           gives lane l chunk r * LPF + l: one 16-byte load of the aligned source chunk
//           that holds the destination chunk's first byte, the following source chunk from
//           the next lane (the group's last lane: from the first lane's load for the next
//           round, which is issued before the current round is consumed), a byte funnel
//           shift by (src_off - 6) mod 16, the tail masked to zero, the chunk's 16-bit
//           words added to the lane's sum (v_dot2_u32_u16), one 16-byte non-temporal store.
//
// Every store instruction of a group writes whole 64-byte lines (LPF >= 4, NC a multiple of
// 4).  The first line (the 54 header bytes and payload bytes 0-9) is kept in the registers of
// the group's lanes 0-3 and stored last, when the group's sum has given the TCP checksum.
// Lanes past the frame's end, and the last round's look-ahead, load the payload's last chunk
// again (first chunk: lanes 0-2 of round 0): loads are issued unconditionally, as
// rxg_rx_frames.h's are and for its reason.  Nothing outside the chunks overlapping the
// payload is read.  What the repeats cost in memory traffic is not separated: the counted
// read traffic of 2^20 x 1460 B segments is 1.18x the algorithmic read bytes,
// which also holds the memory lines at a segment's two ends that its neighbours' groups
// fetch as well; that the repeats themselves are served by the CU's cache is supposed.
//
// Roofline: HBM, algorithmic bytes per segment = data_len (read) + 32 (descriptor) +
// 64 * ceil((54 + data_len) / 64) (written) + 2 (len).
//
// rxg_tx_build_opt_dev is the same kernel instantiated with OPT = true: a segment may carry
// O = 0, 4, .. 40 option bytes from a table of 48-byte blocks (rxg_tx_opt) between the TCP
// header and its payload.  With H = 54 + O (even, so a chunk's 16-bit words stay the
// checksum's words) everything above holds with H for 54: NC = 4 * ceil((H + L) / 64), which
// also gives the size class (one line: H + L <= 64, O <= 8 only); chunk c >= 3 takes its
// payload from the aligned source chunk at ((src_off + 48 - H) & ~15) + 16 * (c - 3) with
// shift (src_off + 10 - O) mod 16, masked to frame bytes [H, H + L).  The option bytes never
// travel between lanes: a block's three 16-byte chunks are the images of frame chunks 3, 4
// and 5 (rxg.h), so the lane that owns one of those chunks loads it aligned (issued with the
// lane's first payload load), masks it to frame bytes [54, H) and ORs it into the chunk
// before the chunk is summed and stored.  For O >= 12 the second line begins with option
// bytes and is stored in the stream like any other line.  A segment without data reads
// nothing of the payload (a streamed frame can have L == 0 here: O >= 12).  The OPT = false
// instantiation is the kernel as it was.  Algorithmic bytes: + 48 per distinct block, and
// 64 * ceil((H + data_len) / 64) written.
#include <type_traits>

#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

constexpr uint32_t kHdr = 54;  // Ethernet 14 + IPv4 20 + TCP 20 (data_off 0x50 without options)

struct TbArgs {
    const uint8_t *payload;
    uint64_t payload_bytes;
    const rxg_tx_flow *flows;
    const rxg_tx_seg *segs;
    uint8_t *frames;
    const uint32_t *off64;  // nullptr: frame i at slot slot0 + i * stride64
    uint16_t *len;
    unsigned long long *stats;
    uint32_t nflows, n, slot0, stride64, nslices;
};

struct TbArgsOpt : TbArgs {
    const rxg_tx_opt *opts;
    uint32_t nopts;
};

template <bool OPT>
using Args = std::conditional_t<OPT, TbArgsOpt, TbArgs>;

// A segment's descriptor and flow record as its lane (and, broadcast, its group) holds them.
struct Seg {
    uint32_t s_lo, s_hi;  // src_off
    uint32_t lw;          // data_len | win_raw << 16
    uint32_t seq, ack;
    uint32_t idf;         // ip_id | tcp_flags << 16 (OPT: | O << 24, the option bytes)
    uint32_t opt;         // OPT: rxg_tx_seg.reserved, the block's index + 1 (unused otherwise)
    uint32_t off;         // 64-byte slot of the frame
    uint32_t ports;       // dport | sport << 16
    uint32_t ip_src_raw;  // rxg_tx_flow.ipv4_dst: the frame's src_addr as stored
    uint32_t ip_dst_host; // rxg_tx_flow.ipv4_src: htonl() of it is the frame's dst_addr
    uint32_t m0, m1, m2;  // frame bytes 0-11: dst MAC, src MAC
};

__device__ __forceinline__ uint32_t hsum(uint32_t d) { return (d & 0xFFFFu) + (d >> 16); }

// The option bytes of a segment (OPT; 0 otherwise) and its headers' length.
template <bool OPT>
__device__ __forceinline__ uint32_t opt_len(const Seg &g)
{
    if constexpr (OPT) return g.idf >> 24;
    else return 0u;
}

template <bool OPT>
__device__ __forceinline__ uint32_t hdr_len(const Seg &g) { return kHdr + opt_len<OPT>(g); }

// Frame chunk c >= 3 from the source chunks lo || hi: the payload bytes it holds, zero
// elsewhere (frame bytes before H = 54 + O: 48-53 of chunk 3 and the option bytes, and bytes
// at or past H + L).
template <bool OPT>
__device__ __forceinline__ uint4 payload_chunk(uint4 lo, uint4 hi, uint32_t sh, uint32_t c, uint32_t L, uint32_t H)
{
    uint4 o = sh ? funnel16(lo, hi, sh) : lo;
    const int vb = (int)(H + L) - (int)(16u * c);
    if (vb < 16) {
        o.x = keep_bytes(o.x, vb);
        o.y = keep_bytes(o.y, vb - 4);
        o.z = keep_bytes(o.z, vb - 8);
        o.w = keep_bytes(o.w, vb - 12);
    }
    if constexpr (OPT) {
        const int hb = (int)H - (int)(16u * c);  // > 0 in chunks 3, 4 (O >= 12) and 5 (O >= 28) only
        if (hb > 0) {
            o.x = drop_bytes(o.x, hb);
            o.y = drop_bytes(o.y, hb - 4);
            o.z = drop_bytes(o.z, hb - 8);
            o.w = drop_bytes(o.w, hb - 12);
        }
    } else if (c == 3u) {
        o.x = 0u;
        o.y &= 0xFFFF0000u;
    }
    return o;
}

// The 16-byte chunk c - 3 of a segment's option block (the image of frame chunk c, c = 3, 4,
// 5: rxg.h) masked to the option bytes, frame bytes [54, H).
__device__ __forceinline__ uint4 option_chunk(uint4 v, uint32_t c, uint32_t H)
{
    const int hb = (int)H - (int)(16u * c);
    v.x = keep_bytes(v.x, hb);
    v.y = keep_bytes(v.y, hb - 4);
    v.z = keep_bytes(v.z, hb - 8);
    v.w = keep_bytes(v.w, hb - 12);
    if (c == 3u) {
        v.x = 0u;
        v.y &= 0xFFFF0000u;
    }
    return v;
}

// Which chunk of its segment's block a lane of a group of LPF loads: that of the one frame
// chunk among 3, 4, 5 the lane owns (LPF 4: lane 3 in round 0, lanes 0 and 1 in round 1),
// 3 or more = none.
template <int LPF>
__device__ __forceinline__ uint32_t option_chunk_of(int gl)
{
    return LPF == 4 ? ((uint32_t)gl + 1u) & 3u : (uint32_t)gl - 3u;
}

// Chunk oc of block k - 1 if it holds option bytes of a block of O bytes (frame bytes 48 +
// 16 oc up to 54 + O), else zeros and no load.  A plain load: segments share blocks.
template <bool OPT>
__device__ __forceinline__ uint4 load_option_chunk(const Args<OPT> &a, uint32_t k, uint32_t O, uint32_t oc)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (OPT) {
        if (O != 0u && oc < 3u && 16u * oc < 6u + O)
            v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const uint8_t *>(a.opts + (k - 1u)) + 16u * oc);
    }
    return v;
}

// Chunk c < 4 of the frame's first line: the headers of etherout.c:87-99, ip.c:97-118 and
// tcp_out.c:174-193 with both checksums, `pay` the sum of the whole segment's option and
// payload bytes (16-bit little-endian words) and p3 chunk 3's part of them (payload_chunk,
// option_chunk).
template <bool OPT>
__device__ __forceinline__ uint4 header_chunk(const Seg &g, uint32_t c, uint32_t pay, uint4 p3)
{
    const uint32_t O = opt_len<OPT>(g);
    const uint32_t L = (g.lw & 0xFFFFu) + O, win = g.lw >> 16;  // L: what follows the 20-byte TCP header
    const uint32_t ipid = g.idf & 0xFFFFu, flags = (g.idf >> 16) & 0xFFu;
    const uint32_t dst = bswap32(g.ip_dst_host), src = g.ip_src_raw;
    const uint32_t seq = bswap32(g.seq), ack = bswap32(g.ack);
    const uint32_t sp = bswap16(g.ports & 0xFFFFu), dp = bswap16(g.ports >> 16);
    // little-endian dwords of frame bytes 12.. : ether_type 08 00, version_ihl 0x45, tos 0
    const uint32_t h3 = 0x00450008u;
    const uint32_t h4 = bswap16((40u + L) & 0xFFFFu) | (ipid << 16);  // total_length, packet_id raw
    const uint32_t h5 = 0x067F0000u;                                 // fragment_offset 0, ttl 127, proto 6
    // both sums over little-endian 16-bit words; the stored field is the folded sum's
    // complement as it stands (htons(calculate_checksum(..)), ip.c:107,118)
    const uint32_t isum = 0x0045u + hsum(h4) + hsum(h5) + hsum(src) + hsum(dst);
    const uint32_t ipck = (~fold16(isum)) & 0xFFFFu;
    const uint32_t h11 = (ack >> 16) | ((0x50u + (O << 2)) << 16) | (flags << 24);  // data_off (5 + O / 4) << 4
    // pseudo {src, dst, 0, 6, htons(20 + L)} || TCP header (cksum, urp 0) || options || payload
    const uint32_t tsum = pay + hsum(src) + hsum(dst) + 0x0600u + bswap16((20u + L) & 0xFFFFu) + sp + dp +
                          hsum(seq) + hsum(ack) + (h11 >> 16) + win;
    const uint32_t tck = (~fold16(tsum)) & 0xFFFFu;
    if (c == 0u) return make_uint4(g.m0, g.m1, g.m2, h3);
    if (c == 1u) return make_uint4(h4, h5, ipck | (src << 16), (src >> 16) | (dst << 16));
    if (c == 2u) return make_uint4((dst >> 16) | (sp << 16), dp | (seq << 16), (seq >> 16) | (ack << 16), h11);
    return make_uint4(win | (tck << 16), p3.y, p3.z, p3.w);
}

// First source address the frame's chunk 3 takes bytes from, rounded down to 16 (may lie
// before the payload's first chunk: loads are clamped to [lo, hi], the chunks that overlap
// the payload), relative to the payload base.
struct Span {
    int64_t base, lo, hi;
    uint32_t sh;
};

template <bool OPT>
__device__ __forceinline__ Span span_of(const Seg &g)
{
    const uint64_t s = ((uint64_t)g.s_hi << 32) | g.s_lo;
    const uint32_t L = g.lw & 0xFFFFu;
    const uint32_t O = opt_len<OPT>(g);
    Span p;
    p.base = ((int64_t)s - 6 - (int64_t)O) & ~15ll;
    p.lo = (int64_t)(s & ~15ull);
    p.hi = (int64_t)((s + L - 1u) & ~15ull);  // (L > 0)
    p.sh = (uint32_t)(s + 10u - O) & 15u;
    return p;
}

// A frame of one line (H + L <= 64: L <= 10 - O), 4 lanes: lane 3 loads what the payload
// touches and, of a block of 4 or 8 bytes, its first chunk.
template <bool OPT>
__device__ __forceinline__ void frame_small(const Args<OPT> &a, const Seg &g, int lane)
{
    const uint32_t c = (uint32_t)lane & 3u;
    const uint32_t L = g.lw & 0xFFFFu;
    const uint32_t O = opt_len<OPT>(g);
    uint4 p3 = make_uint4(0u, 0u, 0u, 0u);
    uint32_t pay = 0;
    if (c == 3u && L != 0u) {
        const Span p = span_of<OPT>(g);
        uint4 A = make_uint4(0u, 0u, 0u, 0u), N = A;
        if (p.base >= p.lo) A = ld16(a.payload + p.base);
        if (p.base + 16 >= p.lo && p.base + 16 <= p.hi) N = ld16(a.payload + p.base + 16);
        p3 = payload_chunk<OPT>(A, N, p.sh, 3u, L, kHdr + O);
        pay = hsum(p3.y) + hsum(p3.z) + hsum(p3.w);
    }
    if constexpr (OPT) {
        if (c == 3u && O != 0u) {
            const uint4 q = option_chunk(load_option_chunk<OPT>(a, g.opt, O, 0u), 3u, kHdr + O);
            p3.y |= q.y; p3.z |= q.z; p3.w |= q.w;
            pay += hsum(q.y) + hsum(q.z) + hsum(q.w);
        }
    }
    st16(a.frames + (size_t)g.off * 64u + 16u * c, header_chunk<OPT>(g, c, pay, p3));
}

template <bool OPT, int LPF>
__device__ __forceinline__ void frame_stream(const Args<OPT> &a, const Seg &g, int lane)
{
    const int gl = lane & (LPF - 1), gbase = lane - gl;
    const uint32_t L = g.lw & 0xFFFFu;  // > 10 (OPT: any, with H + L > 64)
    const uint32_t H = hdr_len<OPT>(g);
    const uint32_t NC = 4u * ((H + L + 63u) >> 6);
    const Span p = span_of<OPT>(g);
    uint8_t *dst = a.frames + (size_t)g.off * 64u;
    // OPT: the clamp as 32-bit offsets from p.base (lo - base <= 48, hi - base < 2^16 + 64)
    const uint8_t *src = a.payload + p.base;
    const int dlo = (int)(p.lo - p.base), dhi = (int)(p.hi - p.base);
    auto load = [&](uint32_t c) -> uint4 {
        if constexpr (OPT) {
            if (L == 0u) return make_uint4(0u, 0u, 0u, 0u);  // a segment without data reads nothing of the payload
            const int o = 16 * ((int)c - 3);
            return ld16(src + (o < dlo ? dlo : o > dhi ? dhi : o));
        } else {
            const int64_t o = p.base + 16ll * ((int64_t)c - 3);
            return ld16(a.payload + (o < p.lo ? p.lo : o > p.hi ? p.hi : o));
        }
    };
    const int from = gl == LPF - 1 ? gbase : lane + 1;
    uint32_t t[4] = {0u, 0u, 0u, 0u};
    uint4 first = make_uint4(0u, 0u, 0u, 0u);
    uint4 cur = load((uint32_t)gl);
    // OPT: this lane's chunk of the block, in flight with its first payload chunk
    const uint4 ov = load_option_chunk<OPT>(a, g.opt, H - kHdr, option_chunk_of<LPF>(gl));
    for (uint32_t c0 = 0; c0 < NC; c0 += (uint32_t)LPF) {
        const uint32_t c = c0 + (uint32_t)gl;
        const uint4 nxt = load(c + (uint32_t)LPF);
        // the source chunk after this lane's: the next lane's, or for the group's last lane
        // the first lane's next
        const uint4 put = gl == 0 ? nxt : cur;
        uint4 N;
        N.x = lane_read(put.x, from);
        N.y = lane_read(put.y, from);
        N.z = lane_read(put.z, from);
        N.w = lane_read(put.w, from);
        uint4 o = payload_chunk<OPT>(cur, N, p.sh, c, L, H);
        if (c < 3u) o = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (OPT) {
            if (c - 3u < 3u) {  // the one chunk of 3, 4, 5 this lane owns: ov is its image
                const uint4 q = option_chunk(ov, c, H);
                o.x |= q.x; o.y |= q.y; o.z |= q.z; o.w |= q.w;
            }
        }
        t[0] = dsum(o.x, t[0]);
        t[1] = dsum(o.y, t[1]);
        t[2] = dsum(o.z, t[2]);
        t[3] = dsum(o.w, t[3]);
        if (c < 4u) first = o;
        else if (c < NC) st16(dst + 16u * c, o);
        cur = nxt;
    }
    const uint32_t pay = lane_read(group_sum<LPF>(t[0] + t[1] + t[2] + t[3], lane), gbase);
    if (gl < 4) st16(dst + 16u * (uint32_t)gl, header_chunk<OPT>(g, (uint32_t)gl, pay, first));
}

// Lanes per frame of a segment of HL = H + L bytes: 0 = frame_small, else frame_stream<LPF>.
__device__ __forceinline__ int class_of(uint32_t HL)
{
    const uint32_t nc = 4u * ((HL + 63u) >> 6);
    return nc <= 4u ? 0 : nc <= 16u ? 4 : nc <= 32u ? 8 : nc <= 64u ? 16 : nc <= 128u ? 32 : 64;
}

// The slice's segments of class CLS (lanes with cls == CLS), 64 / LPF per round.
template <bool OPT, int CLS>
__device__ __forceinline__ void run_class(const Args<OPT> &a, int cls, const Seg &mine, int lane_in)
{
    constexpr int LPF = CLS ? CLS : 4;
    constexpr uint32_t FPW = 64 / LPF;
    const unsigned long long m = __ballot(cls == CLS);
    if (m == 0ull) return;
    int lane = lane_in;
    asm volatile("" : "+v"(lane));  // per-class lane math stays inside the class (VGPRs)
    const uint32_t cnt = (uint32_t)__popcll(m);
    // this class's lanes compacted to 0..cnt-1, keeping their order
    uint32_t corig = (uint32_t)lane;
    if (m != ~0ull) {
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        const uint32_t to = (cls == CLS) ? below : cnt + ((uint32_t)lane - below);
        corig = (uint32_t)__builtin_amdgcn_ds_permute((int)(to << 2), lane);
    }
    for (uint32_t r = 0; r < cnt; r += FPW) {
        const uint32_t k = r + (uint32_t)(lane / LPF);
        const int src = (int)lane_read(corig, (int)(k & 63u));
        Seg g;
        g.s_lo = lane_read(mine.s_lo, src);
        g.s_hi = lane_read(mine.s_hi, src);
        g.lw = lane_read(mine.lw, src);
        g.seq = lane_read(mine.seq, src);
        g.ack = lane_read(mine.ack, src);
        g.idf = lane_read(mine.idf, src);
        g.off = lane_read(mine.off, src);
        g.ports = lane_read(mine.ports, src);
        g.ip_src_raw = lane_read(mine.ip_src_raw, src);
        g.ip_dst_host = lane_read(mine.ip_dst_host, src);
        g.m0 = lane_read(mine.m0, src);
        g.m1 = lane_read(mine.m1, src);
        g.m2 = lane_read(mine.m2, src);
        if constexpr (OPT) g.opt = lane_read(mine.opt, src);
        else g.opt = 0u;
        if (k < cnt) {  // uniform over the group
            if constexpr (CLS == 0) frame_small<OPT>(a, g, lane);
            else frame_stream<OPT, LPF>(a, g, lane);
        }
    }
}

template <bool OPT>
__global__ __launch_bounds__(256) void tx_build_kernel(Args<OPT> a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    uint32_t built = 0, skipped = 0;
    for (uint32_t s = wave; s < a.nslices; s += nwaves) {
        const uint32_t i = s * 64u + (uint32_t)lane;
        const bool inb = i < a.n;
        Seg g = {};
        uint32_t flow = 0;
        if (inb) {  // (8-byte loads: rxg_tx_seg needs 8-byte alignment only)
            const uint2 *d = reinterpret_cast<const uint2 *>(a.segs + i);
            const uint2 d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
            g.s_lo = d0.x; g.s_hi = d0.y;
            flow = d1.x; g.seq = d1.y;
            g.ack = d2.x; g.lw = d2.y;
            g.idf = d3.x & 0x00FFFFFFu;
            if constexpr (OPT) g.opt = d3.y;
        }
        const uint64_t so = ((uint64_t)g.s_hi << 32) | g.s_lo;
        const uint32_t L = g.lw & 0xFFFFu;
        uint32_t O = 0;
        bool valid = inb && flow < a.nflows && L <= RXG_TX_MAX_DATA && so <= a.payload_bytes &&
                     (uint64_t)L <= a.payload_bytes - so;
        if constexpr (OPT) {
            bool opt_ok = g.opt <= a.nopts;  // a block is read only once its index is known to be inside the table
            if (opt_ok && g.opt != 0u) {
                O = *reinterpret_cast<const uint32_t *>(a.opts + (g.opt - 1u)) & 0xFFu;  // rxg_tx_opt.len
                opt_ok = O <= 40u && (O & 3u) == 0u;
                if (!opt_ok) O = 0u;
            }
            g.idf |= O << 24;
            valid = valid && opt_ok && L <= RXG_TX_MAX_DATA - O;
        }
        if (valid) {
            const uint2 *f = reinterpret_cast<const uint2 *>(a.flows + flow);
            const uint2 f0 = f[0], f1 = f[1], f2 = f[2];
            g.ports = f0.x; g.ip_src_raw = f0.y;
            g.ip_dst_host = f1.x; g.m0 = f1.y;
            g.m1 = f2.x; g.m2 = f2.y;
            g.off = frame_slot(a.off64, a.slot0, a.stride64, i);
        }
        if (inb) a.len[i] = valid ? (uint16_t)(kHdr + O + L) : (uint16_t)0;
        built += (uint32_t)__popcll(__ballot(valid));
        skipped += (uint32_t)__popcll(__ballot(inb && !valid));
        const int cls = valid ? class_of(kHdr + O + L) : -1;
        run_class<OPT, 0>(a, cls, g, lane);
        run_class<OPT, 4>(a, cls, g, lane);
        run_class<OPT, 8>(a, cls, g, lane);
        run_class<OPT, 16>(a, cls, g, lane);
        run_class<OPT, 32>(a, cls, g, lane);
        run_class<OPT, 64>(a, cls, g, lane);
    }
    // one atomic instruction per wave: lane 0 adds the built count, lane 1 the skipped
    if (a.stats && lane < 2 && (built | skipped) != 0u)
        atomicAdd(a.stats + lane, (unsigned long long)(lane == 0 ? built : skipped));
}

}  // namespace

int tx_build_blocks_per_cu(bool with_opts)
{
    int n = 0;
    const hipError_t e = with_opts ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tx_build_kernel<true>, 256, 0)
                                   : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tx_build_kernel<false>, 256, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

hipError_t launch_tx_build(const LaunchTxBuild &B, hipStream_t st)
{
    if (B.n == 0) return hipSuccess;
    TbArgsOpt a;
    a.payload = B.payload;
    a.payload_bytes = B.payload_bytes;
    a.flows = B.flows;
    a.segs = B.segs;
    a.frames = B.frames;
    a.off64 = B.off64;
    a.len = B.len;
    a.stats = B.stats;
    a.nflows = B.nflows;
    a.n = B.n;
    a.slot0 = B.slot0;
    a.stride64 = B.stride64;
    a.nslices = (uint32_t)(((uint64_t)B.n + 63u) / 64u);
    uint32_t blocks = (a.nslices + 3u) / 4u;
    if (B.max_blocks && blocks > B.max_blocks) blocks = B.max_blocks;
    a.opts = B.opts;
    a.nopts = B.nopts;
    if (B.with_opts) hipLaunchKernelGGL(tx_build_kernel<true>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tx_build_kernel<false>, dim3(blocks), dim3(256), 0, st, static_cast<const TbArgs &>(a));
    return hipGetLastError();
}

}  // namespace rxg
