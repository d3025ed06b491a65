// rxg_trainpay.hip — a burst's payload gathered by train on the device (rxg_train_payload_dev;
// the rule is stated in rxg.h, its host form is rxg_trainpay.cpp).
//
// msgs zeroed, then four launches on the stream.  No workgroup waits on another, there is no
// ticket and no look-back; every offset is a prefix sum of the arguments, so the grid changes
// nothing.  The grids are sized from n (the host does not read count); a workgroup whose tile
// lies past S' or T' has nothing to do.
//   tp_sizes   a lane per train: the padded size of a taking train, else 0; per tile of kTpTile
//              trains their sum
//   tp_scan    one workgroup: the tile sums -> exclusive prefix sums in place, kTpScanLanes a
//              round with a carry between rounds; the total is *arena_used
//   tp_place   the same sizes again, scanned inside the tile on top of the tile's base: the
//              train's offset (toff[k]; ~0 where the train does not take part or does not fit)
//              and its tmsgs entry
//   tp_copy    a workgroup per tile of kTpTile consecutive entries of `order`.  Its first
//              segment's train is found by a 64-ary search over trains[].first (wave 0, at most
//              four probes deep); the trains that start inside the tile are the next ones, each
//              marks its start in LDS and a scan of the marks gives every lane its train.  A
//              lane then decodes its segment (candidate or hole, source, destination) and the
//              tile's work is cut into items: one per 16-byte destination chunk a segment
//              touches, one per train pad.  An LDS scan of the item counts lays them out in a
//              row; lane l takes items l, l + 256, ... and finds each item's segment by a
//              binary search in that row, so a 65 481-byte segment beside 1-byte ones is shared
//              by the whole workgroup.  A chunk a segment fills whole is two aligned 16-byte
//              loads, a funnel shift and one 16-byte store; a chunk it shares with its
//              neighbours in the train gets only the segment's own bytes, by dword or byte
//              stores, and the pad its zeros likewise: no two items write the same byte.
//
// Roofline: HBM, algorithmic bytes = 2 x payload (read + write) + per segment 4 (order) + the
// record + 16 (frame line for seq and data_off) + 16 (message) + per train 2 x 32 (train, read
// by tp_sizes and tp_place) + 32 (the copy's reads) + 8 + 8 (toff) + 16 (tmsgs).
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

typedef unsigned long long u64;
constexpr u64 kNoOff = ~0ull;

struct TpArgs {
    FrameSrc src;
    const uint8_t *recs;
    const uint32_t *order;
    const rxg_flow_train *trains;
    const u64 *count;
    u64 cap_seg, cap_trains, arena_cap;
    uint8_t *arena;
    rxg_payload_msg *msgs, *tmsgs;
    u64 *used;
    u64 *toff;       // max_trains entries
    u64 *tsum;       // ttiles entries
    uint32_t n, rec_kind, flags;
    uint32_t max_trains, max_segs;  // min(n, cap_trains), min(n, cap_seg): T' and S' never exceed them
    uint32_t ttiles, stiles;        // tiles of max_trains trains, of max_segs segments
};

// S' and T' (rxg.h): min(count, cap, n), which is what the scratch and the grids are sized for.
__device__ __forceinline__ void tp_bounds(const TpArgs &a, uint32_t *S, uint32_t *T)
{
    const u64 c0 = a.count[0], c1 = a.count[1];
    const u64 s = c0 < a.max_segs ? c0 : a.max_segs, t = c1 < a.max_trains ? c1 : a.max_trains;
    *S = (uint32_t)s;
    *T = s ? (uint32_t)t : 0u;
}

__device__ __forceinline__ rxg_flow_train tp_train(const TpArgs &a, uint32_t k)
{
    const uint2 *p = reinterpret_cast<const uint2 *>(a.trains + k);  // (the array is 8-byte aligned)
    const uint2 w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
    rxg_flow_train t;
    t.tcb_idx = (int32_t)w0.x;
    t.first = w0.y;
    t.nseg = w1.x;
    t.seq = w1.y;
    t.bytes = (u64)w2.x | ((u64)w2.y << 32);
    t.next_ack = w3.x;
    t.flags = w3.y;
    return t;
}

// the padded size of train t if it takes part, else 0 with *takes false
__device__ __forceinline__ u64 tp_size(const TpArgs &a, const rxg_flow_train &t, uint32_t S, bool *takes)
{
    *takes = (u64)t.first + t.nseg <= S && t.bytes <= 0xFFFFFFFFull &&
             (!(a.flags & RXG_TP_HEAD_ONLY) || (t.flags & RXG_FTR_HEAD));
    return *takes ? (t.bytes + 15ull) & ~15ull : 0ull;
}

template <bool PLACE>
__device__ __forceinline__ void tp_trains(const TpArgs &a)
{
    __shared__ u64 wsum[kTpTile / 64];
    uint32_t S, T;
    tp_bounds(a, &S, &T);
    for (uint32_t t = blockIdx.x; t < a.ttiles; t += gridDim.x) {
        const uint32_t k0 = t * kTpTile;
        if (k0 >= T) {  // (uniform over the workgroup)
            if (!PLACE && threadIdx.x == 0u) a.tsum[t] = 0ull;
            continue;
        }
        const uint32_t k = k0 + threadIdx.x;
        bool takes = false;
        rxg_flow_train tr = {};
        if (k < T) tr = tp_train(a, k);
        const u64 sz = k < T ? tp_size(a, tr, S, &takes) : 0ull;
        const BlockScan<u64> b = block_scan<u64, kTpTile>(sz, wsum);
        if (!PLACE) {
            if (threadIdx.x == 0u) a.tsum[t] = b.total;
        } else if (k < T) {
            const u64 off = a.tsum[t] + b.before + b.inc - sz;
            const bool placed = takes && off + sz <= a.arena_cap;
            a.toff[k] = placed ? off : kNoOff;
            if (a.tmsgs) {
                rxg_payload_msg m;
                m.arena_off = placed ? off : 0ull;
                m.len = placed ? (uint32_t)tr.bytes : 0u;
                m.flags = placed ? (uint32_t)RXG_PM_GATHERED : 0u;
                a.tmsgs[k] = m;
            }
        }
    }
}

__global__ __launch_bounds__(kTpTile) void tp_sizes(TpArgs a) { tp_trains<false>(a); }
__global__ __launch_bounds__(kTpTile) void tp_place(TpArgs a) { tp_trains<true>(a); }

__global__ __launch_bounds__(kTpScanLanes) void tp_scan(TpArgs a)
{
    __shared__ u64 wsum[kTpScanLanes / 64];
    uint32_t S, T;
    tp_bounds(a, &S, &T);
    const uint32_t nt = (uint32_t)(((u64)T + kTpTile - 1u) / kTpTile);  // (<= ttiles)
    u64 carry = 0;
    for (uint32_t base = 0; base < nt; base += kTpScanLanes) {
        const uint32_t e = base + threadIdx.x;
        const u64 v = e < nt ? a.tsum[e] : 0ull;
        const BlockScan<u64> b = block_scan<u64, kTpScanLanes>(v, wsum);
        if (e < nt) a.tsum[e] = carry + b.before + b.inc - v;
        carry += b.total;
    }
    if (threadIdx.x == 0u) *a.used = carry;
}

// Bytes [b0, b1) of the 16-byte chunk at p written from o, nothing else: a dword store where a
// whole dword lies inside, byte stores at the edges.
__device__ __forceinline__ void store_part(uint8_t *p, uint4 o, uint32_t b0, uint32_t b1)
{
    const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        const uint32_t at = 4u * q;
        if (b0 <= at && at + 4u <= b1) {
            *reinterpret_cast<uint32_t *>(p + at) = w[q];
        } else {
#pragma unroll
            for (uint32_t b = 0; b < 4u; ++b)
                if (at + b >= b0 && at + b < b1) p[at + b] = (uint8_t)(w[q] >> (8u * b));
        }
    }
}

struct TpSeg {
    u64 src;   // byte offset of the payload in the frame pool
    u64 dst;   // byte offset in the arena
    uint32_t len;  // 0: nothing to copy
};

// Segment `pkt` of train tr, placed at off: what to copy, and its message.
__device__ __forceinline__ TpSeg tp_segment(const TpArgs &a, uint32_t pkt, const rxg_flow_train &tr, u64 off)
{
    TpSeg s{0ull, 0ull, 0u};
    if (pkt >= a.n) return s;
    const uint8_t *r = a.recs + (size_t)pkt * a.rec_kind;
    RecFields f;
    if (a.rec_kind == RXG_REC8) f = rec8_fields(*reinterpret_cast<const uint2 *>(r));
    else f = rec16_fields(*reinterpret_cast<const uint4 *>(r));
    const uint32_t flen = a.src.len[pkt];
    if (f.verdict > RXG_V_RST_LISTEN_NONSYN || f.datalen <= 0 || (f.flags & RXG_F_TRUNC) || flen <= 46u) return s;
    const u64 base = (u64)frame_slot(a.src, pkt) * 64ull;
    // bytes 32..47 of the frame (len > 46: inside its first slot): seq at 38, data_off at 46
    const uint4 c = ld16(a.src.frames + base + 32u);
    const uint32_t start = RXG_OFF_TCP + ((c.w >> 20) & 0xFu) * 4u, dl = (uint32_t)f.datalen;
    const uint32_t seq = a.rec_kind == RXG_REC48 ? *reinterpret_cast<const uint32_t *>(r + 24)
                                                 : __builtin_bswap32((c.y >> 16) | (c.z << 16));
    const uint32_t rel = seq - tr.seq;
    if ((u64)start + dl > flen || (u64)rel + dl > tr.bytes) return s;
    s.src = base + start;
    s.dst = off + rel;
    s.len = dl;
    if (a.msgs) {
        rxg_payload_msg m;
        m.arena_off = s.dst;
        m.len = dl;
        // GetData asserts (Length - offset) < 1000, its stack buffer's size (tcp_windows.c:170)
        m.flags = RXG_PM_GATHERED | (dl >= 1000u ? RXG_PM_REF_OVERSIZE : 0u);
        a.msgs[pkt] = m;
    }
    return s;
}

__device__ __forceinline__ uint32_t tp_chunks(u64 dst, uint32_t len)
{
    return len ? (uint32_t)(((dst + len - 1ull) >> 4) - (dst >> 4)) + 1u : 0u;
}

__global__ __launch_bounds__(kTpTile) void tp_copy(TpArgs a)
{
    __shared__ uint32_t wsum[kTpTile / 64];
    __shared__ uint32_t s_t0;
    __shared__ uint32_t s_mark[kTpTile], s_cstart[kTpTile], s_len[kTpTile];
    __shared__ u64 s_src[kTpTile], s_dst[kTpTile], s_pad[kTpTile];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t S, T;
    tp_bounds(a, &S, &T);
    if (T == 0u) return;
    for (uint32_t t = blockIdx.x; t < a.stiles; t += gridDim.x) {
        const uint32_t j0 = t * kTpTile;
        if (j0 >= S) continue;  // (uniform over the workgroup)
        // the last train that starts at or before j0: 64 probes a step, every value wave-uniform
        if (tid < 64u) {
            uint32_t lo = 0, hi = T;
            while (hi - lo > 1u) {
                const uint32_t step = (hi - lo + 63u) / 64u;
                const u64 p = (u64)lo + (u64)lane * step;
                const bool ok = p < hi && a.trains[p].first <= j0;
                const u64 m = __ballot(ok);
                const uint32_t top = m ? 63u - (uint32_t)__builtin_clzll(m) : 0u;
                lo += top * step;
                hi = (u64)lo + step < hi ? lo + step : hi;
            }
            if (lane == 0u) s_t0 = lo;
        }
        s_mark[tid] = 0u;
        __syncthreads();
        const uint32_t t0 = s_t0;
        {   // the trains that start inside the tile are the next ones, at most kTpTile - 1 of them
            const u64 kk = (u64)t0 + 1ull + tid;
            if (kk < T) {
                const uint32_t f = a.trains[kk].first;
                if (f > j0 && f - j0 < kTpTile) s_mark[f - j0] = 1u;
            }
        }
        __syncthreads();
        const BlockScan<uint32_t> ms = block_scan<uint32_t, kTpTile>(s_mark[tid], wsum);
        const u64 k = (u64)t0 + ms.before + ms.inc;
        const uint32_t j = j0 + tid;
        TpSeg seg{0ull, 0ull, 0u};
        u64 pad = 0;  // where a train's pad starts (never a multiple of 16); 0: none of this lane's
        if (j < S && k < T) {
            const rxg_flow_train tr = tp_train(a, (uint32_t)k);
            const u64 off = a.toff[k];
            if (off != kNoOff && j >= tr.first && j - tr.first < tr.nseg) {
                seg = tp_segment(a, a.order[j], tr, off);
                if (seg.len == 0u && a.tmsgs) atomicOr(&a.tmsgs[k].flags, (uint32_t)RXG_PM_HOLE);
                if (j - tr.first == tr.nseg - 1u && (tr.bytes & 15ull)) pad = off + tr.bytes;
            }
        }
        const uint32_t items = tp_chunks(seg.dst, seg.len) + (pad ? 1u : 0u);
        const BlockScan<uint32_t> cs = block_scan<uint32_t, kTpTile>(items, wsum);
        s_cstart[tid] = cs.before + cs.inc - items;
        s_len[tid] = seg.len;
        s_src[tid] = seg.src;
        s_dst[tid] = seg.dst;
        s_pad[tid] = pad;
        __syncthreads();
        for (uint32_t idx = tid; idx < cs.total; idx += kTpTile) {
            uint32_t s = 0;  // the last segment whose row starts at or before idx
#pragma unroll
            for (uint32_t step = kTpTile / 2u; step; step >>= 1)
                if (s_cstart[s + step] <= idx) s += step;
            const uint32_t q = idx - s_cstart[s], L = s_len[s];
            const u64 d = s_dst[s];
            if (q < tp_chunks(d, L)) {
                const u64 cA = ((d >> 4) + q) << 4;
                const u64 lo = cA > d ? cA : d, hi = cA + 16ull < d + L ? cA + 16ull : d + L;
                // the source byte that belongs at cA (before the payload for a first partial chunk:
                // never before byte 19 of the frame, the payload starts at 34 or later)
                const u64 sa = s_src[s] + cA - d;
                const u64 ab = sa & ~15ull;
                const uint32_t sh = (uint32_t)(sa & 15ull);
                const u64 ns = sa + (lo - cA), ne = sa + (hi - cA);  // the source bytes needed
                // each load holds a needed byte, so it lies inside the slots the frame's len occupies
                uint4 A = make_uint4(0u, 0u, 0u, 0u), B = A;
                if (ns < ab + 16ull) A = ld16(a.src.frames + ab);
                if (ne > ab + 16ull) B = ld16(a.src.frames + ab + 16ull);
                const uint4 o = funnel16(A, B, sh);
                if (hi - lo == 16ull) st16(a.arena + cA, o);
                else store_part(a.arena + cA, o, (uint32_t)(lo - cA), (uint32_t)(hi - cA));
            } else {
                const u64 p = s_pad[s];
                store_part(a.arena + (p & ~15ull), make_uint4(0u, 0u, 0u, 0u), (uint32_t)(p & 15ull), 16u);
            }
        }
        __syncthreads();  // the rows are rewritten by the next tile
    }
}

inline uint32_t tp_tiles(uint32_t entries) { return (uint32_t)(((uint64_t)entries + kTpTile - 1u) / kTpTile); }
inline uint32_t tp_max_trains(uint32_t n, unsigned long long cap_trains) { return cap_trains < n ? (uint32_t)cap_trains : n; }

}  // namespace

size_t train_pay_scratch_bytes(uint32_t n, unsigned long long cap_trains)
{
    const uint32_t mt = tp_max_trains(n, cap_trains);
    return ((size_t)mt + tp_tiles(mt) + 1u) * sizeof(u64);
}

int train_pay_blocks_per_cu()
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, tp_copy, (int)kTpTile, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

hipError_t launch_train_pay(const LaunchTrainPay &P, hipStream_t st)
{
    hipError_t e = hipSuccess;
    if (P.n == 0) return hipMemsetAsync(P.used, 0, sizeof(u64), st);
    if (P.msgs && (e = hipMemsetAsync(P.msgs, 0, (size_t)P.n * sizeof(rxg_payload_msg), st)) != hipSuccess) return e;
    TpArgs a;
    a.src = P.src;
    a.recs = P.recs;
    a.order = P.order;
    a.trains = P.trains;
    a.count = P.count;
    a.cap_seg = P.cap_seg;
    a.cap_trains = P.cap_trains;
    a.arena_cap = P.arena_cap;
    a.arena = P.arena;
    a.msgs = P.msgs;
    a.tmsgs = P.tmsgs;
    a.used = P.used;
    a.n = P.n;
    a.rec_kind = P.rec_kind;
    a.flags = P.flags;
    a.max_trains = tp_max_trains(P.n, P.cap_trains);
    a.max_segs = P.cap_seg < P.n ? (uint32_t)P.cap_seg : P.n;
    a.ttiles = tp_tiles(a.max_trains);
    a.stiles = tp_tiles(a.max_segs);
    a.toff = reinterpret_cast<u64 *>(P.scratch);
    a.tsum = a.toff + a.max_trains;
    const uint32_t cap = P.max_blocks ? P.max_blocks : 1u << 16;
    const uint32_t tblocks = std::max(std::min(a.ttiles, cap), 1u), sblocks = std::min(a.stiles, cap);
    hipLaunchKernelGGL(tp_sizes, dim3(tblocks), dim3(kTpTile), 0, st, a);
    hipLaunchKernelGGL(tp_scan, dim3(1), dim3(kTpScanLanes), 0, st, a);
    if (a.ttiles) hipLaunchKernelGGL(tp_place, dim3(tblocks), dim3(kTpTile), 0, st, a);
    if (sblocks) hipLaunchKernelGGL(tp_copy, dim3(sblocks), dim3(kTpTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace rxg
