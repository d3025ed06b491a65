// rxg_txreset.hip — reset replies built on the device from a burst's records
// (rxg_tx_reset_dev).
//
// What the reference does per offending packet on the CPU -- send_reset (tcp_out.c:103-146: a
// fresh buffer, the TCP header mirrored from the offender's) -> ip_out (ip.c:62-132: the IPv4
// header, two mallocs, two byte-loop checksums) -> ether_out (etherout.c:87-99) -- for every
// frame of a burst whose record says RXG_V_RST_NOPCB or RXG_V_RST_LISTEN_NONSYN.  A reset is
// a pure function of the offender's first line and a running packet id, so the only thing
// the frames share is their order: reset k belongs to the k-th such frame.
//
// Three launches on the stream, no workgroup waits on another:
//   tx_reset_count   a wave per 64-frame slice (grid-stride): ballot of the RST verdicts,
//                    counts[slice] = its popcount
//   tx_reset_scan    one workgroup: counts[] -> its exclusive prefix sums in place, and
//                    *count = the total
//   tx_reset_build   a wave per slice again: the same ballot; a frame's rank is its slice's
//                    base + the ballot bits below its lane.  The slice's RST lanes store
//                    idx[rank] = i (one coalesced store), then the slice's resets are built
//                    4 lanes per reset, 16 resets per round: lane c of a group loads chunk c
//                    (16 bytes) of the offender's first line masked by len[i] (chunk 3 holds
//                    nothing a reset uses: lane 3 issues no load), the group's lanes get
//                    chunks 1 and 2 by DPP quad broadcasts, every lane forms its 16 bytes of
//                    the reset, adds their 16-bit words to the two checksums' partial sums
//                    (v_dot2_u32_u16), the group's sums come from a DPP reduction, and each
//                    lane issues one 16-byte non-temporal store: a group writes one line.
//                    Lanes of other frames load no frame bytes.
// The output depends on the records only, never on the grid.
//
// Roofline: HBM, algorithmic bytes = 2 * n * record size (the records are read by the count
// and by the build pass) + per reset 64 (read) + 64 (written) + 4 (idx).
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

struct TrArgs {
    FrameSrc src;
    const uint8_t *recs;
    uint8_t *out;
    uint32_t *idx;
    unsigned long long cap;
    uint32_t *counts;       // nslices entries: the count pass's counts, then their prefix sums
    uint32_t n, nslices, rec_kind;
    uint32_t ip_id0;
    uint32_t m0, m1;        // src_mac bytes 0-3, 4-5
};

__device__ __forceinline__ bool is_rst(const TrArgs &a, uint32_t i)
{
    const uint32_t v = rec_verdict(a.recs, a.rec_kind, i);
    return v == RXG_V_RST_NOPCB || v == RXG_V_RST_LISTEN_NONSYN;
}

__global__ __launch_bounds__(256) void tx_reset_count(TrArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    for (uint32_t s = wave; s < a.nslices; s += nwaves) {
        const uint32_t i = s * 64u + lane;
        const unsigned long long m = __ballot(i < a.n && is_rst(a, i));
        if (lane == 0u) a.counts[s] = (uint32_t)__popcll(m);
    }
}

// counts[0 .. nslices) -> exclusive prefix sums in place, *count = the total.  One workgroup
// of 1024 lanes; a lane takes 16 consecutive entries (the buffer is a whole number of
// 16-entry groups: entries at or past nslices count as 0, what is stored there is unused).
constexpr uint32_t kScanLanes = 1024, kScanPer = 16;
__global__ __launch_bounds__(1024) void tx_reset_scan(uint32_t *counts, uint32_t nslices, unsigned long long *count)
{
    __shared__ uint32_t wsum[kScanLanes / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nslices; base += kScanLanes * kScanPer) {
        const uint32_t e0 = base + threadIdx.x * kScanPer;
        uint32_t v[kScanPer] = {};
        uint32_t t = 0;
        if (e0 < nslices) {
            const uint4 *p = reinterpret_cast<const uint4 *>(counts + e0);
#pragma unroll
            for (uint32_t q = 0; q < kScanPer / 4u; ++q) {
                const uint4 w = p[q];
                v[4 * q] = w.x; v[4 * q + 1] = w.y; v[4 * q + 2] = w.z; v[4 * q + 3] = w.w;
            }
#pragma unroll
            for (uint32_t j = 0; j < kScanPer; ++j) {
                if (e0 + j >= nslices) v[j] = 0u;
                t += v[j];
            }
        }
        const BlockScan<uint32_t> b = block_scan<uint32_t, kScanLanes>(t, wsum);
        if (e0 < nslices) {
            uint32_t run = carry + b.before + b.inc - t;
            uint4 *p = reinterpret_cast<uint4 *>(counts + e0);
#pragma unroll
            for (uint32_t q = 0; q < kScanPer / 4u; ++q) {
                uint4 w;
                w.x = run; run += v[4 * q];
                w.y = run; run += v[4 * q + 1];
                w.z = run; run += v[4 * q + 2];
                w.w = run; run += v[4 * q + 3];
                p[q] = w;
            }
        }
        carry += b.total;
    }
    if (threadIdx.x == 0u) *count = carry;
}

// The 16 bytes lane c of a group stores for reset number K (chunk c of the line), and its
// part of the two checksums' sums: *ip over line bytes 14-33, *tcp over the pseudo header
// {src, dst, 0, 6, htons(20)} and bytes 34-53, both as sums of little-endian 16-bit words
// with the checksum fields zero (the stored field is the folded sum's complement as it
// stands, htons(calculate_checksum(..)), ip.c:107,118).  in0: the offender's chunk 0 (lane
// 0's load); c1z .. c2w: dwords 2-3 of its chunk 1 and 0-3 of its chunk 2.
__device__ __forceinline__ uint4 reset_chunk(const TrArgs &a, uint32_t c, uint32_t K, uint4 in0, uint32_t c1z,
                                             uint32_t c1w, uint32_t c2x, uint32_t c2y, uint32_t c2z, uint32_t c2w,
                                             uint32_t *ip, uint32_t *tcp)
{
    const uint32_t src = (c1z >> 16) | (c1w << 16);   // in[26..30), the offender's src_addr
    const uint32_t dst = (c1w >> 16) | (c2x << 16);   // in[30..34), its dst_addr
    const uint32_t ack = (c2z >> 16) | (c2w << 16);   // in[42..46), its recv_ack
    uint4 o;
    if (c == 0u) {
        // in[6..12) || src_mac || 08 00 || version_ihl 0x45, tos 0
        o = make_uint4((in0.y >> 16) | (in0.z << 16), (in0.z >> 16) | (a.m0 << 16), (a.m0 >> 16) | (a.m1 << 16),
                       0x00450008u);
        *ip = dsum(o.w & 0xFFFF0000u, 0u);
        *tcp = 0u;
    } else if (c == 1u) {
        // total_length htons(40), packet_id raw; fragment_offset 0, ttl 127, proto 6;
        // hdr_checksum (filled in by the caller), src_addr = the offender's dst_addr; dst_addr
        o = make_uint4(0x00002800u | (((a.ip_id0 + K) & 0xFFFFu) << 16), 0x067F0000u, dst << 16,
                       (dst >> 16) | (src << 16));
        *ip = dsum(o.w, dsum(o.z, dsum(o.y, dsum(o.x, 0u))));
        *tcp = dsum(o.w, dsum(o.z, 0u));
    } else if (c == 2u) {
        // dst_addr's second half; src_port = in[36..38), dst_port = in[34..36); sent_seq = the
        // offender's recv_ack; recv_ack 0; data_off 0x50, RST
        o = make_uint4((src >> 16) | (c2y << 16), (c2x >> 16) | (ack << 16), ack >> 16,
                       0x04500000u);
        *ip = dsum(o.x & 0xFFFFu, 0u);
        *tcp = dsum(o.w, dsum(o.z, dsum(o.y, dsum(o.x, 0u))));
    } else {
        // rx_win 12000 unswapped, cksum (filled in by the caller), tcp_urp 0, bytes 54-63 zero
        o = make_uint4(12000u, 0u, 0u, 0u);
        *ip = 0u;
        *tcp = dsum(o.x, 0x0600u + 0x1400u);  // pseudo: protocol 6, htons(20)
    }
    return o;
}

__global__ __launch_bounds__(256) void tx_reset_build(TrArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    const uint32_t c = lane & 3u;
    for (uint32_t s = wave; s < a.nslices; s += nwaves) {
        const uint32_t i = s * 64u + lane;
        const bool rst = i < a.n && is_rst(a, i);
        const unsigned long long m = __ballot(rst);
        if (m == 0ull) continue;
        const uint32_t base = a.counts[s], cnt = (uint32_t)__popcll(m);
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        uint32_t off = 0, ln = 0;
        if (rst) {
            off = frame_slot(a.src, i);
            ln = a.src.len[i];
            if ((unsigned long long)base + below < a.cap) a.idx[(size_t)base + below] = i;
        }
        // the slice's RST lanes compacted to 0 .. cnt-1, keeping their order
        uint32_t corig = lane;
        if (m != ~0ull) {
            const uint32_t to = rst ? below : cnt + (lane - below);
            corig = (uint32_t)__builtin_amdgcn_ds_permute((int)(to << 2), (int)lane);
        }
        for (uint32_t r = 0; r < cnt; r += 16u) {
            const uint32_t k = r + (lane >> 2);
            const int from = (int)lane_read(corig, (int)(k & 63u));
            const uint32_t goff = lane_read(off, from);
            const int glen = (int)lane_read(ln, from);
            const unsigned long long K = (unsigned long long)base + k;
            const bool act = k < cnt && K < a.cap;  // uniform over the group
            uint4 in = make_uint4(0u, 0u, 0u, 0u);
            if (act && c < 3u) {
                in = ld16(a.src.frames + (size_t)goff * 64u + 16u * c);
                const int vb = glen - (int)(16u * c);  // bytes at and beyond len read as zero
                if (vb < 16) {
                    in.x = keep_bytes(in.x, vb);
                    in.y = keep_bytes(in.y, vb - 4);
                    in.z = keep_bytes(in.z, vb - 8);
                    in.w = keep_bytes(in.w, vb - 12);
                }
            }
            const uint32_t c1z = quad_bcast<1>(in.z), c1w = quad_bcast<1>(in.w);
            const uint32_t c2x = quad_bcast<2>(in.x), c2y = quad_bcast<2>(in.y);
            const uint32_t c2z = quad_bcast<2>(in.z), c2w = quad_bcast<2>(in.w);
            uint32_t ip, tcp;
            uint4 o = reset_chunk(a, c, (uint32_t)K, in, c1z, c1w, c2x, c2y, c2z, c2w, &ip, &tcp);
            // the group's sums, valid in its first lane, handed to the lanes that store them
            ip += dpp_down<1>(ip);
            tcp += dpp_down<1>(tcp);
            ip += dpp_down<2>(ip);
            tcp += dpp_down<2>(tcp);
            ip = quad_bcast<0>(ip);
            tcp = quad_bcast<0>(tcp);
            if (c == 1u) o.z |= (~fold16(ip)) & 0xFFFFu;
            if (c == 3u) o.x |= ((~fold16(tcp)) & 0xFFFFu) << 16;
            if (act) st16(a.out + (size_t)K * 64u + 16u * c, o);
        }
    }
}

}  // namespace

int tx_reset_blocks_per_cu()
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tx_reset_build, 256, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

size_t tx_reset_count_bytes(uint32_t n)
{
    const size_t nslices = ((size_t)n + 63u) / 64u;
    return (nslices + kScanPer - 1u) / kScanPer * kScanPer * sizeof(uint32_t);
}

hipError_t launch_tx_reset(const LaunchTxReset &R, hipStream_t st)
{
    if (R.n == 0) return hipMemsetAsync(R.count, 0, sizeof(unsigned long long), st);
    TrArgs a;
    a.src = R.src;
    a.recs = R.recs;
    a.out = R.out;
    a.idx = R.idx;
    a.cap = R.cap;
    a.counts = R.counts;
    a.n = R.n;
    a.nslices = (uint32_t)(((uint64_t)R.n + 63u) / 64u);
    a.rec_kind = R.rec_kind;
    a.ip_id0 = R.ip_id0;
    a.m0 = (uint32_t)R.src_mac[0] | ((uint32_t)R.src_mac[1] << 8) | ((uint32_t)R.src_mac[2] << 16) |
           ((uint32_t)R.src_mac[3] << 24);
    a.m1 = (uint32_t)R.src_mac[4] | ((uint32_t)R.src_mac[5] << 8);
    uint32_t blocks = (a.nslices + 3u) / 4u;
    if (R.max_blocks && blocks > R.max_blocks) blocks = R.max_blocks;
    hipLaunchKernelGGL(tx_reset_count, dim3(blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(tx_reset_scan, dim3(1), dim3(kScanLanes), 0, st, a.counts, a.nslices, R.count);
    hipLaunchKernelGGL(tx_reset_build, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace rxg
