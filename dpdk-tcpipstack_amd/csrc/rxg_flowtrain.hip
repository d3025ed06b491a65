// rxg_flowtrain.hip — a burst's data segments grouped by flow and cut into in-order trains on
// the device (rxg_flow_trains_dev; the rule is stated in rxg.h, its host form is
// rxg_flowtrain.cpp).
//
// Three steps, 7 + 3 * passes launches on the stream; no workgroup waits on another and no step
// takes an atomic, so every rank is a function of the arguments alone and the grid changes
// nothing.  The grids are sized from n (the host does not know S); a workgroup whose tile lies
// past S has nothing to do.
//   select   ft_select_count  a wave per 64-frame slice decodes the records: per slice the
//                             number of segments, of DISPATCH records out of range and of
//                             frames left out by the checksum flag
//            ft_scan (select) one workgroup: segment counts -> exclusive prefix sums in place,
//                             S and count[0], count[2], count[3]
//            ft_select_write  a wave per slice again: a segment's rank is its slice's base +
//                             the ballot bits below its lane; pairs[rank] = (tcb_idx, packet
//                             index), and meta[packet index] = (seq, datalen | FIN << 16),
//                             the only place a frame byte is read
//   sort     a least-significant-digit radix sort of the pairs on tcb_idx, 8 bits a pass, as
//            many passes as ntcb - 1 has bytes.  A tile is kFtTile pairs: a workgroup of 256
//            lanes takes it in four rounds, so a tile has 16 wave-rounds in list order.
//            ft_hist          per wave-round, eight ballots give each lane the set of lanes
//                             with its digit; the lowest of them writes the set's size into
//                             an LDS table [wave-round][digit]; lane d sums column d into
//                             hist[d * ntiles + tile] (digit-major)
//            ft_scan (plain)  hist[] -> exclusive prefix sums in place: where each (digit,
//                             tile) goes
//            ft_scatter       the same table; lane d turns column d into running positions
//                             from hist's base, a pair goes to its wave-round's position +
//                             the same-digit lanes below it.  The last pass also writes
//                             order[]
//   cut      ft_cut_count     a lane per sorted pair: "starts a train" from its own and its
//                             predecessor's pair and meta; per tile the number of starts
//            ft_scan (cut)    tile counts -> exclusive prefix sums, T and count[1],
//                             starts[T] = S
//            ft_cut_write     the same test; starts[rank] = the pair's position
//            ft_emit          a lane per train: its segments are [starts[r], starts[r + 1]).
//                             Inside a train no segment wraps and each starts where the one
//                             before ended, so bytes = seq_last - seq_first + datalen_last
//                             with no sum over the segments
//
// Roofline: HBM, algorithmic bytes = 2 * n * record size + per segment 16 (frame line, 8- and
// 16-byte records) + 8 (meta) + passes * 32 (pairs read twice, written once per pass) + 4
// (order) + cut 2 * (8 + 16 gathered) + per train 4 + 32.
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

struct FtHdr {              // device words the launches hand on
    uint32_t S, T;
};

struct FtArgs {
    FrameSrc src;           // (frames and len unused for RXG_REC48)
    const uint8_t *recs;
    const uint32_t *cur_seq;
    uint32_t *order;
    rxg_flow_train *trains;
    unsigned long long cap_seg, cap_trains;
    unsigned long long *count;
    uint2 *pairs[2];        // n entries each: (tcb_idx, packet index)
    uint2 *meta;            // n entries by packet index: (seq, datalen | FIN << 16)
    uint32_t *starts;       // n + 1 entries: the position in the sorted list each train starts at
    uint32_t *cnt_seg, *cnt_out, *cnt_left;  // per slice
    uint32_t *hist;         // 256 * ntiles, digit-major
    uint32_t *cuts;         // per tile
    FtHdr *hdr;
    uint32_t n, nslices, ntiles, rec_kind, ntcb, flags;
};

enum : uint32_t { kNone, kSeg, kOut, kLeft };
constexpr uint32_t kFinBit = 1u << 16;

// What frame i is to the rule (i < n), with its tcb_idx, datalen and FIN.
__device__ __forceinline__ uint32_t ft_decode(const FtArgs &a, uint32_t i, int32_t *tcb, uint32_t *dlfin)
{
    const uint8_t *r = a.recs + (size_t)i * a.rec_kind;
    RecFields f;
    if (a.rec_kind == RXG_REC8) f = rec8_fields(*reinterpret_cast<const uint2 *>(r));
    else f = rec16_fields(*reinterpret_cast<const uint4 *>(r));
    *tcb = f.tcb_idx;
    *dlfin = ((uint32_t)f.datalen & 0xFFFFu) | ((f.tcp_flags & 1u) ? kFinBit : 0u);
    if (f.verdict != RXG_V_DISPATCH) return kNone;
    if (f.tcb_idx < 0 || (uint32_t)f.tcb_idx >= a.ntcb) return kOut;
    if ((a.flags & RXG_FT_TCP_OK_ONLY) && !(f.flags & RXG_F_TCP_OK)) return kLeft;
    return (f.datalen > 0 && f.datalen <= 65535) ? kSeg : kNone;
}

__global__ __launch_bounds__(256) void ft_select_count(FtArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    for (uint32_t s = wave; s < a.nslices; s += nwaves) {
        const uint32_t i = s * 64u + lane;
        int32_t tcb;
        uint32_t dlfin;
        const uint32_t k = i < a.n ? ft_decode(a, i, &tcb, &dlfin) : (uint32_t)kNone;
        const uint32_t cs = (uint32_t)__popcll(__ballot(k == kSeg)), co = (uint32_t)__popcll(__ballot(k == kOut)),
                       cl = (uint32_t)__popcll(__ballot(k == kLeft));
        if (lane == 0u) {
            a.cnt_seg[s] = cs;
            a.cnt_out[s] = co;
            a.cnt_left[s] = cl;
        }
    }
}

// v[0 .. len) -> exclusive prefix sums in place.  One workgroup of kFtScanLanes lanes; a lane
// takes kFtScanPer consecutive entries (the buffer is a whole number of such groups: entries
// at or past len count as 0, what is stored there is unused).  What else the workgroup does:
//   kScanSelect  S = the total -> hdr and count[0]; count[2], count[3] = the sums of the two
//                other per-slice counts
//   kScanPlain   nothing
//   kScanCut     T = the total -> hdr and count[1]; starts[T] = S
enum : uint32_t { kScanSelect, kScanPlain, kScanCut };
__global__ __launch_bounds__(1024) void ft_scan(FtArgs a, uint32_t *v, uint32_t len, uint32_t what)
{
    __shared__ uint32_t wsum[kFtScanLanes / 64];
    __shared__ unsigned long long wsum2[kFtScanLanes / 64];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < len; base += kFtScanLanes * kFtScanPer) {
        const uint32_t e0 = base + threadIdx.x * kFtScanPer;
        uint32_t x[kFtScanPer] = {};
        uint32_t t = 0;
        if (e0 < len) {
            const uint4 *p = reinterpret_cast<const uint4 *>(v + e0);
#pragma unroll
            for (uint32_t q = 0; q < kFtScanPer / 4u; ++q) {
                const uint4 w = p[q];
                x[4 * q] = w.x; x[4 * q + 1] = w.y; x[4 * q + 2] = w.z; x[4 * q + 3] = w.w;
            }
#pragma unroll
            for (uint32_t j = 0; j < kFtScanPer; ++j) {
                if (e0 + j >= len) x[j] = 0u;
                t += x[j];
            }
        }
        const BlockScan<uint32_t> b = block_scan<uint32_t, kFtScanLanes>(t, wsum);
        if (e0 < len) {
            uint32_t run = carry + b.before + b.inc - t;
            uint4 *p = reinterpret_cast<uint4 *>(v + e0);
#pragma unroll
            for (uint32_t q = 0; q < kFtScanPer / 4u; ++q) {
                uint4 w;
                w.x = run; run += x[4 * q];
                w.y = run; run += x[4 * q + 1];
                w.z = run; run += x[4 * q + 2];
                w.w = run; run += x[4 * q + 3];
                p[q] = w;
            }
        }
        carry += b.total;
    }
    if (what == kScanSelect) {
        // the two left-out counters: plain sums over the slices (64-bit: n may reach 2^32 - 1)
        unsigned long long o = 0, l = 0;
        for (uint32_t s = threadIdx.x; s < len; s += kFtScanLanes) {
            o += a.cnt_out[s];
            l += a.cnt_left[s];
        }
        const BlockScan<unsigned long long> bo = block_scan<unsigned long long, kFtScanLanes>(o, wsum2);
        const BlockScan<unsigned long long> bl = block_scan<unsigned long long, kFtScanLanes>(l, wsum2);
        if (threadIdx.x == 0u) {
            a.hdr->S = carry;
            a.count[0] = carry;
            a.count[2] = bo.total;
            a.count[3] = bl.total;
        }
    } else if (what == kScanCut) {
        if (threadIdx.x == 0u) {
            a.hdr->T = carry;
            a.count[1] = carry;
            a.starts[carry] = a.hdr->S;  // (T <= S <= n: starts has n + 1 entries)
        }
    }
}

__global__ __launch_bounds__(256) void ft_select_write(FtArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    for (uint32_t s = wave; s < a.nslices; s += nwaves) {
        const uint32_t i = s * 64u + lane;
        int32_t tcb = 0;
        uint32_t dlfin = 0;
        const bool seg = i < a.n && ft_decode(a, i, &tcb, &dlfin) == kSeg;
        const unsigned long long m = __ballot(seg);
        if (m == 0ull) continue;
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (!seg) continue;
        uint32_t seq = 0;
        if (a.rec_kind == RXG_REC48) {
            seq = *reinterpret_cast<const uint32_t *>(a.recs + (size_t)i * RXG_REC48 + 24);
        } else {
            const int ln = (int)a.src.len[i];
            if (ln > 38) {  // a byte of seq lies inside the frame: its first line is readable
                const uint4 c = ld16(a.src.frames + (size_t)frame_slot(a.src, i) * 64u + 32u);
                const uint32_t y = keep_bytes(c.y, ln - 36), z = keep_bytes(c.z, ln - 40);
                seq = __builtin_bswap32((y >> 16) | (z << 16));
            }
        }
        const uint32_t rank = a.cnt_seg[s] + below;
        // (rank < S <= n always; the guard keeps a wrong rank, should one ever be computed, from
        // writing outside the scratch of a device others share -- the slot it should have written
        // then stays stale and the output compare fails all the same)
        if (rank < a.n) a.pairs[0][rank] = make_uint2((uint32_t)tcb, i);
        a.meta[i] = make_uint2(seq, dlfin);
    }
}

// ------------------------------------------------------------------------ the sort ---
// The lanes of the wave that hold digit d's value, as a mask (`valid` lanes only; a lane that
// is not valid gets 0): eight ballots, one per bit.
__device__ __forceinline__ unsigned long long same_digit(uint32_t d, bool valid)
{
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; ++b) {
        const unsigned long long set = __ballot((d >> b) & 1u);
        m &= ((d >> b) & 1u) ? set : ~set;
    }
    return valid ? m : 0ull;
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

constexpr uint32_t kFtRounds = kFtTile / 256u;   // rounds a workgroup takes a tile in
constexpr uint32_t kFtSubs = kFtRounds * 4u;     // wave-rounds of a tile, in list order

// SCATTER false: hist[d * ntiles + t] = the pairs of tile t whose digit is d.
// SCATTER true: hist holds the prefix sums; the pairs move from src to dst (and, LAST, their
// packet indices into order).
template <bool SCATTER, bool LAST>
__device__ __forceinline__ void ft_pass(const FtArgs &a, const uint2 *src, uint2 *dst, uint32_t shift)
{
    __shared__ uint32_t tab[kFtSubs][256];
    const uint32_t wib = threadIdx.x >> 6;
    const uint32_t S = a.hdr->S;
    for (uint32_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint32_t t0 = t * kFtTile;
        if (t0 >= S) {  // (uniform over the workgroup)
            if (!SCATTER) a.hist[(size_t)threadIdx.x * a.ntiles + t] = 0u;
            continue;
        }
#pragma unroll
        for (uint32_t q = 0; q < kFtSubs; ++q) tab[q][threadIdx.x] = 0u;
        __syncthreads();
        uint2 key[kFtRounds];
        uint32_t dig[kFtRounds], below[kFtRounds];
        bool valid[kFtRounds];
#pragma unroll
        for (uint32_t r = 0; r < kFtRounds; ++r) {
            const uint32_t e = t0 + r * 256u + threadIdx.x;
            valid[r] = e < S;
            key[r] = valid[r] ? src[e] : make_uint2(0u, 0u);
            dig[r] = (key[r].x >> shift) & 0xFFu;
            const unsigned long long m = same_digit(dig[r], valid[r]);
            below[r] = lanes_below(m);  // (the same-digit lanes before this one)
            if (valid[r] && below[r] == 0u) tab[r * 4u + wib][dig[r]] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        {
            const uint32_t d = threadIdx.x;
            uint32_t run = SCATTER ? a.hist[(size_t)d * a.ntiles + t] : 0u;
#pragma unroll
            for (uint32_t q = 0; q < kFtSubs; ++q) {
                const uint32_t c = tab[q][d];
                if (SCATTER) tab[q][d] = run;
                run += c;
            }
            if (!SCATTER) a.hist[(size_t)d * a.ntiles + t] = run;
        }
        if (SCATTER) {
            __syncthreads();
#pragma unroll
            for (uint32_t r = 0; r < kFtRounds; ++r) {
                if (!valid[r]) continue;
                const uint32_t pos = tab[r * 4u + wib][dig[r]] + below[r];
                if (pos >= a.n) continue;  // (never: a permutation of [0, S); the guard as in ft_select_write)
                dst[pos] = key[r];
                if (LAST && pos < a.cap_seg) a.order[pos] = key[r].y;
            }
        }
        __syncthreads();  // tab is zeroed again by the next tile
    }
}

__global__ __launch_bounds__(256) void ft_hist(FtArgs a, const uint2 *src, uint32_t shift)
{
    ft_pass<false, false>(a, src, nullptr, shift);
}

__global__ __launch_bounds__(256) void ft_scatter(FtArgs a, const uint2 *src, uint2 *dst, uint32_t shift)
{
    ft_pass<true, false>(a, src, dst, shift);
}

__global__ __launch_bounds__(256) void ft_scatter_last(FtArgs a, const uint2 *src, uint2 *dst, uint32_t shift)
{
    ft_pass<true, true>(a, src, dst, shift);
}

// ------------------------------------------------------------------------- the cut ---
__device__ __forceinline__ bool ft_wraps(uint2 m)
{
    return (unsigned long long)m.x + (m.y & 0xFFFFu) >= (1ull << 32);
}

// Does the sorted list's pair k (< S) start a train?
__device__ __forceinline__ bool ft_starts(const FtArgs &a, const uint2 *sorted, uint32_t k)
{
    if (k == 0u) return true;
    const uint2 p = sorted[k - 1u], q = sorted[k];
    if (p.x != q.x) return true;
    const uint2 ma = a.meta[p.y], mb = a.meta[q.y];
    const bool cont = mb.x == ma.x + (ma.y & 0xFFFFu) && !(ma.y & kFinBit) && !ft_wraps(ma) && !ft_wraps(mb);
    return !cont;
}

template <bool WRITE>
__device__ __forceinline__ void ft_cut(const FtArgs &a, const uint2 *sorted)
{
    __shared__ uint32_t wcnt[kFtSubs];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    const uint32_t S = a.hdr->S;
    for (uint32_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const uint32_t t0 = t * kFtTile;
        if (t0 >= S) {
            if (!WRITE && threadIdx.x == 0u) a.cuts[t] = 0u;
            continue;
        }
        unsigned long long m[kFtRounds];
#pragma unroll
        for (uint32_t r = 0; r < kFtRounds; ++r) {
            const uint32_t k = t0 + r * 256u + threadIdx.x;
            m[r] = __ballot(k < S && ft_starts(a, sorted, k));
            if (lane == 0u) wcnt[r * 4u + wib] = (uint32_t)__popcll(m[r]);
        }
        __syncthreads();
        if (!WRITE) {
            if (threadIdx.x == 0u) {
                uint32_t c = 0;
#pragma unroll
                for (uint32_t q = 0; q < kFtSubs; ++q) c += wcnt[q];
                a.cuts[t] = c;
            }
        } else {
            uint32_t run = a.cuts[t];
#pragma unroll
            for (uint32_t q = 0; q < kFtSubs; ++q) {
                const uint32_t r = q >> 2;
                if ((q & 3u) == wib && ((m[r] >> lane) & 1ull)) {
                    const uint32_t rank = run + lanes_below(m[r]);
                    if (rank < a.n) a.starts[rank] = t0 + r * 256u + threadIdx.x;  // (guard as in ft_select_write)
                }
                run += wcnt[q];
            }
        }
        __syncthreads();  // wcnt is rewritten by the next tile
    }
}

__global__ __launch_bounds__(256) void ft_cut_count(FtArgs a, const uint2 *sorted) { ft_cut<false>(a, sorted); }
__global__ __launch_bounds__(256) void ft_cut_write(FtArgs a, const uint2 *sorted) { ft_cut<true>(a, sorted); }

__global__ __launch_bounds__(256) void ft_emit(FtArgs a, const uint2 *sorted)
{
    const uint32_t S = a.hdr->S, T = a.hdr->T;
    const unsigned long long total = (unsigned long long)gridDim.x * 256u;
    for (unsigned long long r = (unsigned long long)blockIdx.x * 256u + threadIdx.x; r < T && r < a.cap_trains;
         r += total) {
        const uint32_t first = a.starts[r], next = a.starts[r + 1u];
        const uint2 ka = sorted[first], kz = sorted[next - 1u];
        const uint2 ma = a.meta[ka.y], mz = a.meta[kz.y];
        const bool fin = (mz.y & kFinBit) != 0u, wrap = ft_wraps(ma);
        const bool flow_first = first == 0u || sorted[first - 1u].x != ka.x;
        const bool flow_last = next == S || sorted[next].x != ka.x;
        rxg_flow_train o;
        o.tcb_idx = (int32_t)ka.x;
        o.first = first;
        o.nseg = next - first;
        o.seq = ma.x;
        // no segment of a train of several wraps, and each starts where the one before ended
        o.bytes = (unsigned long long)(uint32_t)(mz.x - ma.x) + (mz.y & 0xFFFFu);
        o.next_ack = (uint32_t)(ma.x + o.bytes) + (fin ? 1u : 0u);
        o.flags = (fin ? RXG_FTR_FIN : 0u) | (wrap ? RXG_FTR_WRAP : 0u) | (flow_first ? RXG_FTR_FLOW_FIRST : 0u) |
                  (flow_last ? RXG_FTR_FLOW_LAST : 0u);
        if (flow_first && a.cur_seq && !wrap) {
            const uint32_t cur = a.cur_seq[ka.x];
            if (cur != 0u && cur == ma.x) o.flags |= RXG_FTR_HEAD;
        }
        a.trains[r] = o;
    }
}

inline size_t pad_scan(size_t entries) { return (entries + kFtScanPer - 1u) / kFtScanPer * kFtScanPer; }
inline uint32_t ft_slices(uint32_t n) { return (uint32_t)(((uint64_t)n + 63u) / 64u); }
inline uint32_t ft_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + kFtTile - 1u) / kFtTile); }

}  // namespace

uint32_t flow_train_passes(uint32_t ntcb) { return ntcb - 1u < (1u << 8) ? 1u : ntcb - 1u < (1u << 16) ? 2u : 3u; }

size_t flow_train_pair_bytes(uint32_t n) { return 2u * (size_t)n * sizeof(uint2); }

size_t flow_train_meta_bytes(uint32_t n) { return (size_t)n * sizeof(uint2) + ((size_t)n + 1u) * sizeof(uint32_t); }

size_t flow_train_count_bytes(uint32_t n)
{
    return (16u + 3u * pad_scan(ft_slices(n)) + pad_scan(256u * (size_t)ft_tiles(n)) + pad_scan(ft_tiles(n))) *
           sizeof(uint32_t);
}

int flow_train_blocks_per_cu()
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ft_scatter, 256, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

hipError_t launch_flow_train(const LaunchFlowTrain &F, hipStream_t st)
{
    if (F.n == 0) return hipMemsetAsync(F.count, 0, 4 * sizeof(unsigned long long), st);
    FtArgs a;
    a.src = F.src;
    a.recs = F.recs;
    a.cur_seq = F.cur_seq;
    a.order = F.order;
    a.trains = F.trains;
    a.cap_seg = F.cap_seg;
    a.cap_trains = F.cap_trains;
    a.count = F.count;
    a.n = F.n;
    a.nslices = ft_slices(F.n);
    a.ntiles = ft_tiles(F.n);
    a.rec_kind = F.rec_kind;
    a.ntcb = F.ntcb;
    a.flags = F.flags;
    a.pairs[0] = reinterpret_cast<uint2 *>(F.pairs);
    a.pairs[1] = a.pairs[0] + F.n;
    a.meta = reinterpret_cast<uint2 *>(F.meta);
    a.starts = reinterpret_cast<uint32_t *>(a.meta + F.n);
    uint32_t *w = F.counts;
    a.hdr = reinterpret_cast<FtHdr *>(w);
    w += 16;
    a.cnt_seg = w;
    w += pad_scan(a.nslices);
    a.cnt_out = w;
    w += pad_scan(a.nslices);
    a.cnt_left = w;
    w += pad_scan(a.nslices);
    a.hist = w;
    w += pad_scan(256u * (size_t)a.ntiles);
    a.cuts = w;
    const uint32_t cap = F.max_blocks ? F.max_blocks : 1u << 16;
    const uint32_t sblocks = std::min((a.nslices + 3u) / 4u, cap), tblocks = std::min(a.ntiles, cap),
                   eblocks = std::min((uint32_t)(((uint64_t)F.n + 255u) / 256u), cap);
    hipLaunchKernelGGL(ft_select_count, dim3(sblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(ft_scan, dim3(1), dim3(kFtScanLanes), 0, st, a, a.cnt_seg, a.nslices, (uint32_t)kScanSelect);
    hipLaunchKernelGGL(ft_select_write, dim3(sblocks), dim3(256), 0, st, a);
    const uint32_t passes = flow_train_passes(F.ntcb);
    uint32_t from = 0;
    for (uint32_t p = 0; p < passes; ++p, from ^= 1u) {
        const uint2 *src = a.pairs[from];
        uint2 *dst = a.pairs[from ^ 1u];
        hipLaunchKernelGGL(ft_hist, dim3(tblocks), dim3(256), 0, st, a, src, 8u * p);
        hipLaunchKernelGGL(ft_scan, dim3(1), dim3(kFtScanLanes), 0, st, a, a.hist, 256u * a.ntiles, (uint32_t)kScanPlain);
        if (p + 1u == passes) hipLaunchKernelGGL(ft_scatter_last, dim3(tblocks), dim3(256), 0, st, a, src, dst, 8u * p);
        else hipLaunchKernelGGL(ft_scatter, dim3(tblocks), dim3(256), 0, st, a, src, dst, 8u * p);
    }
    const uint2 *sorted = a.pairs[from];
    hipLaunchKernelGGL(ft_cut_count, dim3(tblocks), dim3(256), 0, st, a, sorted);
    hipLaunchKernelGGL(ft_scan, dim3(1), dim3(kFtScanLanes), 0, st, a, a.cuts, a.ntiles, (uint32_t)kScanCut);
    hipLaunchKernelGGL(ft_cut_write, dim3(tblocks), dim3(256), 0, st, a, sorted);
    hipLaunchKernelGGL(ft_emit, dim3(eblocks), dim3(256), 0, st, a, sorted);
    return hipGetLastError();
}

}  // namespace rxg
