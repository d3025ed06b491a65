// rxg_txplan.hip — sends cut into segment descriptors on the device (rxg_tx_plan_dev).
//
// What rxg_tx_plan_opt does on one host core -- walk every send, write one 32-byte rxg_tx_seg
// per segment -- with the sends (40 bytes each) as the only thing that crosses to the device.
// Every field of segment q of send j is a closed form of the send, q and the cut length
// m_j = mss - O_j; the only ordered part is first[j], the prefix sum of the sends' segment
// counts.
//
// Four launches on the stream, no workgroup waits on another:
//   tx_plan_count    a lane per send, a workgroup per tile of kTile sends (grid-stride): the
//                    send's segment count nseg_j (0 for a refused send), first[j] = its
//                    exclusive prefix inside the tile (a wave scan, then the tile's waves through
//                    LDS), tiles[t] = {the tile's segments, its refused sends}, next_seq[j]
//   tx_plan_scan     one workgroup: tiles[t].segs -> the exclusive prefix sums over the tiles in
//                    place, count = {total, refused}, first[nsends] = total.  64-bit sums.
//   tx_plan_offsets  a lane per send again: first[j] += its tile's base
//   tx_plan_expand   centred on the output: a wave takes 64 consecutive segment indices
//                    k < min(total, cap) (grid-stride), a lane finds its send by an upper-bound
//                    search in first[] (a refused send's two bounds are equal: it is never
//                    found), reads it as 16 + 16 + 8 bytes, forms the descriptor and stores it
//                    as two 16-byte stores: a wave writes 2 KiB contiguous, whatever the spread
//                    of the bytes over the sends.
// The output depends on the arguments only, never on the grid.
//
// Roofline: HBM, algorithmic bytes = per send 40 + 4 (send_opt) read and 8 (first) + 4
// (next_seq) written, per segment 32 written.  The offsets pass (16 per send) and the expand
// pass's search and send reads (served by the caches: neighbouring lanes read the same sends)
// come on top.
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

constexpr uint32_t kTile = 256;        // sends per tile = lanes per workgroup of the count pass
constexpr uint32_t kScanLanes = 1024;  // tiles per round of the scan's loop, one per lane

struct TpArgs {
    const uint8_t *sends;     // nsends rxg_tx_send (40 bytes each, 8-byte aligned)
    const uint32_t *send_opt; // nullptr: no send names a block
    const uint8_t *opts;      // nopts rxg_tx_opt (48 bytes each; byte 0 = len)
    uint8_t *segs;
    unsigned long long cap;
    unsigned long long *first;
    uint32_t *next_seq;       // may be nullptr
    unsigned long long *count;
    ulonglong2 *tiles;        // ntiles entries: {segments, refused sends} of the tile; after the
                              // scan .x is the tile's base
    uint32_t nsends, mss, nopts, ntiles;
};

// (8-byte aligned: sends and descriptors are 40 and 32 bytes at an 8-byte aligned base)
typedef unsigned int u32x4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct Send {
    uint32_t flow, next_seq, ack, bytes, flags, win_id;  // win_id: win_raw | ip_id0 << 16
    unsigned long long src_off;
};

// the 40 bytes of send j as 16 + 16 + 8
__device__ __forceinline__ Send load_send(const uint8_t *sends, uint32_t j)
{
    const uint8_t *p = sends + (size_t)j * 40u;
    const u32x4a8 a = *reinterpret_cast<const u32x4a8 *>(p);
    const u32x4a8 b = *reinterpret_cast<const u32x4a8 *>(p + 16);
    const u32x2 c = *reinterpret_cast<const u32x2 *>(p + 32);
    Send s;
    s.flow = a.x;
    s.next_seq = a.y;
    s.ack = a.z;
    s.src_off = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
    s.bytes = b.z;
    s.flags = b.w & 0xFFu;
    s.win_id = c.x;
    return s;
}

// The cut length m_j = mss - O_j of a send that names block k (0: none), or 0 when the send is
// refused: k > nopts, the block's len over 40 or not a multiple of 4, mss <= O.  The block is
// read only once k <= nopts is established.
__device__ __forceinline__ uint32_t cut_len(const TpArgs &a, uint32_t k)
{
    uint32_t O = 0;
    if (k) {
        if (k > a.nopts) return 0u;
        O = a.opts[(size_t)(k - 1u) * 48u];
        if (O > 40u || (O & 3u)) return 0u;
    }
    return a.mss > O ? a.mss - O : 0u;
}

// Both scans below are the workgroup step of rxg_dev.h's block_scan with a second channel riding
// on its two barriers (the refused sends).  Written out: as two block_scan calls the planner
// measured 58.1 us against 57.1 on 2^20 one-segment sends, outside the runs' 0.7 us spread.
__global__ __launch_bounds__(kTile) void tx_plan_count(TpArgs a)
{
    __shared__ unsigned long long wsum[kTile / 64];
    __shared__ uint32_t wref[kTile / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const unsigned long long j = (unsigned long long)t * kTile + threadIdx.x;
        uint32_t nseg = 0;
        bool refused = false;
        if (j < a.nsends) {
            const Send s = load_send(a.sends, (uint32_t)j);
            const uint32_t m = cut_len(a, a.send_opt ? a.send_opt[j] : 0u);
            refused = m == 0u;
            if (!refused) nseg = s.bytes ? (s.bytes - 1u) / m + 1u : 1u;
            // the sequence number after the send: + bytes, + 1 for SYN, + 1 for FIN
            if (a.next_seq)
                a.next_seq[j] = refused ? s.next_seq
                                        : s.next_seq + s.bytes + ((s.flags & RXG_TCP_FLAG_SYN) ? 1u : 0u) +
                                              ((s.flags & RXG_TCP_FLAG_FIN) ? 1u : 0u);
        }
        const unsigned long long inc = wave_incl_scan<unsigned long long>(nseg, lane);
        const unsigned long long rm = __ballot(refused);
        if (lane == 63u) {
            wsum[wave] = inc;
            wref[wave] = (uint32_t)__popcll(rm);
        }
        __syncthreads();
        unsigned long long before = 0, total = 0;
        uint32_t nref = 0;
#pragma unroll
        for (uint32_t w = 0; w < kTile / 64u; ++w) {
            const unsigned long long x = wsum[w];
            if (w < wave) before += x;
            total += x;
            nref += wref[w];
        }
        __syncthreads();  // wsum is rewritten by the next tile
        if (j < a.nsends) a.first[j] = before + inc - nseg;
        if (threadIdx.x == 0u) a.tiles[t] = make_ulonglong2(total, nref);
    }
}

// tiles[0 .. ntiles).x -> exclusive prefix sums in place; count = {total, refused sends};
// first[nsends] = total.  One workgroup of kScanLanes lanes, a tile per lane and round.
__global__ __launch_bounds__(kScanLanes) void tx_plan_scan(TpArgs a)
{
    __shared__ unsigned long long wsum[kScanLanes / 64], wref[kScanLanes / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = 0, refused = 0;
    for (uint32_t base = 0; base < a.ntiles; base += kScanLanes) {
        const uint32_t e = base + threadIdx.x;  // (ntiles <= 2^24: no wrap)
        ulonglong2 v = make_ulonglong2(0ull, 0ull);
        if (e < a.ntiles) v = a.tiles[e];
        const unsigned long long inc = wave_incl_scan(v.x, lane), rinc = wave_incl_scan(v.y, lane);
        if (lane == 63u) {
            wsum[wave] = inc;
            wref[wave] = rinc;
        }
        __syncthreads();
        unsigned long long before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanLanes / 64u; ++w) {
            const unsigned long long x = wsum[w];
            if (w < wave) before += x;
            total += x;
            refused += wref[w];
        }
        __syncthreads();  // wsum is rewritten by the next round
        if (e < a.ntiles) a.tiles[e].x = carry + before + inc - v.x;
        carry += total;
    }
    if (threadIdx.x == 0u) {
        a.count[0] = carry;
        a.count[1] = refused;
        a.first[a.nsends] = carry;
    }
}

// first[j]: the prefix inside its tile -> the index of send j's first segment
__global__ __launch_bounds__(256) void tx_plan_offsets(TpArgs a)
{
    const unsigned long long step = (unsigned long long)gridDim.x * 256u;
    // (tile 0's base is 0)
    for (unsigned long long j = (unsigned long long)blockIdx.x * 256u + threadIdx.x + kTile; j < a.nsends; j += step)
        a.first[j] += a.tiles[j / kTile].x;
}

__global__ __launch_bounds__(256) void tx_plan_expand(TpArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long wave = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
    const unsigned long long step = (unsigned long long)gridDim.x * 256u;
    const unsigned long long total = a.first[a.nsends];
    const unsigned long long lim = total < a.cap ? total : a.cap;
    for (unsigned long long k = wave * 64u + lane; k < lim; k += step) {
        // the send of segment k: first[j] <= k < first[j + 1]  (first[0] = 0, first[nsends] = total > k)
        uint32_t lo = 0, hi = a.nsends;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (a.first[mid] <= k) lo = mid;
            else hi = mid;
        }
        const uint32_t j = lo;
        const uint32_t q = (uint32_t)(k - a.first[j]);  // nseg_j <= 2^32 - 1
        const bool last = k + 1u == a.first[j + 1u];
        const Send s = load_send(a.sends, j);
        const uint32_t blk = a.send_opt ? a.send_opt[j] : 0u;
        const uint32_t m = cut_len(a, blk);  // (not 0: a refused send has no segment)
        const unsigned long long done = (unsigned long long)q * m;
        const uint32_t len = last ? s.bytes - (uint32_t)done : m;
        const uint32_t once_first = RXG_TCP_FLAG_SYN, once_last = RXG_TCP_FLAG_FIN | RXG_TCP_FLAG_PSH;
        uint32_t fl = s.flags & ~(once_first | once_last);
        if (q == 0u) fl |= s.flags & once_first;
        if (last) fl |= s.flags & once_last;
        const uint32_t seq = s.next_seq + (uint32_t)done + ((q && (s.flags & RXG_TCP_FLAG_SYN)) ? 1u : 0u);
        const uint32_t ip_id = ((s.win_id >> 16) + q) & 0xFFFFu;
        const unsigned long long src = s.src_off + done;
        u32x4a8 o0, o1;
        o0.x = (uint32_t)src;
        o0.y = (uint32_t)(src >> 32);
        o0.z = s.flow;
        o0.w = seq;
        o1.x = s.ack;
        o1.y = (len & 0xFFFFu) | (s.win_id << 16);  // data_len, win_raw
        o1.z = ip_id | (fl << 16);                  // ip_id, tcp_flags, pad 0
        o1.w = blk;                                 // reserved
        uint8_t *p = a.segs + (size_t)k * 32u;
        *reinterpret_cast<u32x4a8 *>(p) = o0;
        *reinterpret_cast<u32x4a8 *>(p + 16) = o1;
    }
}

}  // namespace

int tx_plan_blocks_per_cu()
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tx_plan_expand, 256, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

size_t tx_plan_tile_bytes(uint32_t nsends)
{
    return (((size_t)nsends + kTile - 1u) / kTile) * sizeof(ulonglong2);
}

hipError_t launch_tx_plan(const LaunchTxPlan &P, hipStream_t st)
{
    if (P.nsends == 0) {  // count = {0, 0}, first[0] = 0
        const hipError_t e = hipMemsetAsync(P.count, 0, 2 * sizeof(unsigned long long), st);
        return e != hipSuccess ? e : hipMemsetAsync(P.first, 0, sizeof(unsigned long long), st);
    }
    TpArgs a;
    a.sends = (const uint8_t *)P.sends;
    a.send_opt = P.send_opt;
    a.opts = (const uint8_t *)P.opts;
    a.segs = (uint8_t *)P.segs;
    a.cap = P.cap;
    a.first = P.first;
    a.next_seq = P.next_seq;
    a.count = P.count;
    a.tiles = (ulonglong2 *)P.tiles;
    a.nsends = P.nsends;
    a.mss = P.mss;
    a.nopts = P.nopts;
    a.ntiles = (uint32_t)(((uint64_t)P.nsends + kTile - 1u) / kTile);
    // every pass is grid-stride: without a cap of the caller's, 2^16 workgroups at the most (far
    // inside HIP's grid limits whatever nsends and cap are)
    const uint32_t cap_blocks = P.max_blocks ? P.max_blocks : 1u << 16;
    const uint32_t send_blocks = a.ntiles < cap_blocks ? a.ntiles : cap_blocks;
    hipLaunchKernelGGL(tx_plan_count, dim3(send_blocks), dim3(kTile), 0, st, a);
    hipLaunchKernelGGL(tx_plan_scan, dim3(1), dim3(kScanLanes), 0, st, a);
    if (a.ntiles > 1u) hipLaunchKernelGGL(tx_plan_offsets, dim3(send_blocks), dim3(256), 0, st, a);
    if (P.cap) {
        // min(total, cap) segments are written: cap bounds the grid, only the device knows the
        // total (with a cap far over it the surplus workgroups read first[nsends] and end)
        const unsigned long long need = (P.cap - 1u) / 256u + 1u;
        const uint32_t blocks = need < cap_blocks ? (uint32_t)need : cap_blocks;
        hipLaunchKernelGGL(tx_plan_expand, dim3(blocks), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace rxg
