// rxg_flowsum.hip — a burst summarised per flow on the device from its records and frames
// (rxg_flow_sums_dev; the rule is stated in rxg.h, its host form is rxg_flowsum.cpp).
//
// A segmented reduction keyed by tcb_idx.  The context owns a dense accumulator of ntcb
// entries (FlowSumAcc, 40 bytes each) and a touched bitmap, both all zero between calls:
// "lowest index" is kept as the maximum of ~i and "highest" as the maximum of i + 1, so zero
// means none and nothing is cleared per burst.  Four launches on the stream, no workgroup
// waits on another:
//   flow_sum_acc     a lane per frame, a wave per run of consecutive 64-frame slices.  The
//                    lane decodes its record; a counted frame of an 8- or 16-byte record loads
//                    frame bytes 32..47 once (masked by len) for seq and ack.  Where the
//                    counted lanes of a slice all hold one tcb_idx, each lane folds its frame
//                    into registers it carries from slice to slice, with no cross-lane work
//                    but two ballots; the carried flow is reduced over the wave and added to
//                    memory by one lane only when the flow changes or the wave is done (a
//                    workgroup's waves that end on the same flow are merged through LDS
//                    first).  In every other slice each counted lane issues its own atomics.
//                    All of them are integer max / add / or: the sums are exact in any order.
//   flow_sum_count   a wave per tile of 64 bitmap words: tiles[t] = its set bits
//   flow_sum_scan    one workgroup: tiles[] -> exclusive prefix sums in place, count[0] = the
//                    total, count[1..2] = the two left-out counters, which it zeroes
//   flow_sum_expand  a wave per tile: two bitmap words at a time, lane l takes bit l & 31 of
//                    word 2 k + (l >> 5), so a wave reads 64 consecutive accumulator entries;
//                    rank = tile base + set bits below; out[rank] is written when rank < cap
//                    (state from recs[first_idx]); the entry and the bitmap word are zeroed
//                    for every touched entry, past cap too.
// The output depends on the arguments only, never on the grid.
//
// Roofline: HBM, algorithmic bytes = n * record size + 16 per counted frame (8- and 16-byte
// records) + ntcb / 8 of bitmap + 40 per flow.
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

struct FsArgs {
    FrameSrc src;                // (frames and len unused for RXG_REC48)
    const uint8_t *recs;
    FlowSumAcc *acc;
    uint32_t *bits;              // the bitmap (past the two left-out counters)
    unsigned long long *left;    // {DISPATCH out of range, left out by the checksum flag}
    uint32_t *tiles;
    rxg_flow_sum *out;
    unsigned long long cap;
    unsigned long long *count;
    uint32_t n, nslices, rec_kind, ntcb, flags, ntiles;
};

// One flow's contribution: a frame's, or a wave's carried sum.
struct Part {
    uint32_t frames, max_seq, max_ack, first_enc, last_enc, data_frames, flags_or;
    unsigned long long data_bytes;
};

__device__ __forceinline__ Part part_zero() { return Part{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0ull}; }

__device__ __forceinline__ void part_merge(Part &a, const Part &b)
{
    a.frames += b.frames;
    a.max_seq = max(a.max_seq, b.max_seq);
    a.max_ack = max(a.max_ack, b.max_ack);
    a.first_enc = max(a.first_enc, b.first_enc);
    a.last_enc = max(a.last_enc, b.last_enc);
    a.data_frames += b.data_frames;
    a.flags_or |= b.flags_or;
    a.data_bytes += b.data_bytes;
}

// The wave's lanes' parts reduced into every lane (a butterfly over the 64 lanes).
__device__ __forceinline__ Part part_wave(Part p, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int from = (int)(lane ^ (uint32_t)d);
        Part q;
        q.frames = lane_read(p.frames, from);
        q.max_seq = lane_read(p.max_seq, from);
        q.max_ack = lane_read(p.max_ack, from);
        q.first_enc = lane_read(p.first_enc, from);
        q.last_enc = lane_read(p.last_enc, from);
        q.data_frames = lane_read(p.data_frames, from);
        q.flags_or = lane_read(p.flags_or, from);
        q.data_bytes = (unsigned long long)lane_read((uint32_t)p.data_bytes, from) |
                       ((unsigned long long)lane_read((uint32_t)(p.data_bytes >> 32), from) << 32);
        part_merge(p, q);
    }
    return p;
}

// p added to flow tcb's accumulator entry (tcb < ntcb) and its bit set.  An atomic that would
// change nothing is not issued; the two words that only ever gain bits during the launch are
// read first (a stale read costs one atomic more, never a lost bit).
__device__ __forceinline__ void part_commit(const FsArgs &a, uint32_t tcb, const Part &p)
{
    FlowSumAcc *e = a.acc + tcb;
    atomicAdd(&e->frames, p.frames);
    if (p.max_seq) atomicMax(&e->max_seq, p.max_seq);
    if (p.max_ack) atomicMax(&e->max_ack, p.max_ack);
    atomicMax(&e->first_enc, p.first_enc);
    atomicMax(&e->last_enc, p.last_enc);
    if (p.data_frames) {
        atomicAdd(&e->data_frames, p.data_frames);
        atomicAdd(&e->data_bytes, p.data_bytes);
    }
    if (p.flags_or &&
        (__hip_atomic_load(&e->flags_or, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & p.flags_or) != p.flags_or)
        atomicOr(&e->flags_or, p.flags_or);
    uint32_t *w = a.bits + (tcb >> 5);
    const uint32_t bit = 1u << (tcb & 31u);
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
}

__global__ __launch_bounds__(256) void flow_sum_acc(FsArgs a)
{
    __shared__ Part s_part[4];
    __shared__ int s_flow[4];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    const uint32_t wave = blockIdx.x * 4u + wib, nwaves = gridDim.x * 4u;
    // a wave takes a run of consecutive slices: a flow's frames arrive in trains
    const uint32_t per = (a.nslices + nwaves - 1u) / nwaves;
    const uint32_t s0 = min(wave * per, a.nslices), s1 = min(s0 + per, a.nslices);
    Part carry = part_zero();
    int flow = -1;  // the carried flow (wave-uniform); -1: none
    uint32_t nout = 0, nleft = 0;  // (lane 0's) left-out frames of this wave
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t i = s * 64u + lane;
        const bool in = i < a.n;
        RecFields f = {-1, 0xFFu, 0u, 0u, 0};  // past the burst's end: no verdict
        const uint8_t *r = a.recs + (size_t)i * a.rec_kind;
        if (in) {
            if (a.rec_kind == RXG_REC8) f = rec8_fields(*reinterpret_cast<const uint2 *>(r));
            else f = rec16_fields(*reinterpret_cast<const uint4 *>(r));
        }
        const int32_t tcb = f.tcb_idx, dl = f.datalen;
        const uint32_t verdict = f.verdict, rfl = f.flags, tfl = f.tcp_flags;
        const bool disp = in && verdict == RXG_V_DISPATCH;
        const bool inr = disp && tcb >= 0 && (uint32_t)tcb < a.ntcb;
        const bool ok = !(a.flags & RXG_FS_TCP_OK_ONLY) || (rfl & RXG_F_TCP_OK);
        const bool counted = inr && ok;
        nout += (uint32_t)__popcll(__ballot(disp && !inr));
        nleft += (uint32_t)__popcll(__ballot(inr && !ok));
        const unsigned long long m = __ballot(counted);
        if (m == 0ull) continue;
        uint32_t seq = 0, ack = 0;
        if (counted) {
            if (a.rec_kind == RXG_REC48) {
                const uint2 w = *reinterpret_cast<const uint2 *>(r + 24);
                seq = w.x;
                ack = w.y;
            } else {
                const uint32_t off = frame_slot(a.src, i);
                const int ln = (int)a.src.len[i];
                if (ln > 38) {  // a byte of seq or ack lies inside the frame: its first line is readable
                    const uint4 c = ld16(a.src.frames + (size_t)off * 64u + 32u);  // 64-bit: a pool may pass 4 GiB
                    const uint32_t y = keep_bytes(c.y, ln - 36), z = keep_bytes(c.z, ln - 40),
                                   w = keep_bytes(c.w, ln - 44);
                    seq = __builtin_bswap32((y >> 16) | (z << 16));
                    ack = __builtin_bswap32((z >> 16) | (w << 16));
                }
            }
        }
        Part p = part_zero();
        if (counted) {
            p.frames = 1u;
            p.max_seq = seq;
            p.max_ack = ack;
            p.first_enc = ~i;
            p.last_enc = i + 1u;
            p.data_frames = dl > 0 ? 1u : 0u;
            p.flags_or = tfl;
            p.data_bytes = dl > 0 ? (unsigned long long)dl : 0ull;
        }
        const int first = __builtin_ctzll(m);
        const int t0 = __builtin_amdgcn_readfirstlane((int)lane_read((uint32_t)tcb, first));
        if (__ballot(counted && tcb != t0) == 0ull) {
            if (flow != t0) {
                if (flow >= 0) {
                    const Part w = part_wave(carry, lane);
                    if (lane == 0u) part_commit(a, (uint32_t)flow, w);
                    carry = part_zero();
                }
                flow = t0;
            }
            part_merge(carry, p);  // (a lane that holds no counted frame merges zeroes)
        } else if (counted) {
            part_commit(a, (uint32_t)tcb, p);
        }
    }
    // the workgroup's carried flows: waves that end on the same flow are merged first
    const Part w = part_wave(carry, lane);
    if (lane == 0u) {
        s_part[wib] = w;
        s_flow[wib] = flow;
        if (nout) atomicAdd(&a.left[0], (unsigned long long)nout);
        if (nleft) atomicAdd(&a.left[1], (unsigned long long)nleft);
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (s_flow[k] < 0) continue;
            Part t = s_part[k];
#pragma unroll
            for (int j = k + 1; j < 4; ++j)
                if (s_flow[j] == s_flow[k]) {
                    part_merge(t, s_part[j]);
                    s_flow[j] = -1;
                }
            part_commit(a, (uint32_t)s_flow[k], t);
        }
    }
}

// the set bits of the tile's 64 words, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += lane_read(v, (int)(lane ^ (uint32_t)d));
    return v;
}

__global__ __launch_bounds__(256) void flow_sum_count(FsArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    for (uint32_t t = wave; t < a.ntiles; t += nwaves) {
        const uint32_t c = wave_sum((uint32_t)__popc(a.bits[(size_t)t * kFsTileWords + lane]), lane);
        if (lane == 0u) a.tiles[t] = c;
    }
}

// tiles[0 .. ntiles) -> exclusive prefix sums in place (rxg_dev.h block_scan, one entry per
// lane and round), count[0] = the total; the two left-out counters move to count[1..2] and
// are zeroed for the next call.
__global__ __launch_bounds__(1024) void flow_sum_scan(uint32_t *tiles, uint32_t ntiles, unsigned long long *left,
                                                      unsigned long long *count)
{
    __shared__ uint32_t wsum[kFsScanLanes / 64];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < ntiles; base += kFsScanLanes) {
        const uint32_t e = base + threadIdx.x;
        const uint32_t t = e < ntiles ? tiles[e] : 0u;
        const BlockScan<uint32_t> b = block_scan<uint32_t, kFsScanLanes>(t, wsum);
        if (e < ntiles) tiles[e] = (uint32_t)carry + b.before + b.inc - t;
        carry += b.total;
    }
    if (threadIdx.x == 0u) {
        count[0] = carry;
        count[1] = left[0];
        count[2] = left[1];
        left[0] = 0ull;
        left[1] = 0ull;
    }
}

__global__ __launch_bounds__(256) void flow_sum_expand(FsArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    const uint32_t bit = lane & 31u;
    for (uint32_t t = wave; t < a.ntiles; t += nwaves) {
        uint32_t *wp = a.bits + (size_t)t * kFsTileWords + lane;
        const uint32_t w = *wp;
        if (__ballot(w != 0u) == 0ull) continue;
        // set bits in the tile's words before this lane's
        const uint32_t pc = (uint32_t)__popc(w);
        const uint32_t excl = wave_incl_scan(pc, lane) - pc;
        const unsigned long long base = a.tiles[t];
        for (uint32_t k = 0; k < kFsTileWords / 2u; ++k) {
            const int src = (int)(2u * k + (lane >> 5));
            const uint32_t ww = lane_read(w, src), ee = lane_read(excl, src);
            if (__ballot(ww != 0u) == 0ull) continue;
            const uint32_t tcb = (t * kFsTileWords + (uint32_t)src) * 32u + bit;
            if (!((ww >> bit) & 1u) || tcb >= a.ntcb) continue;
            const unsigned long long rank = base + ee + (uint32_t)__popc(ww & ((1u << bit) - 1u));
            FlowSumAcc *e = a.acc + tcb;
            const FlowSumAcc v = *e;
            if (rank < a.cap) {
                const uint32_t fi = ~v.first_enc;
                uint32_t st = RXG_STATE_NONE;
                if (fi < a.n) {
                    const uint8_t *r = a.recs + (size_t)fi * a.rec_kind;
                    if (a.rec_kind == RXG_REC8) {
                        st = (*reinterpret_cast<const uint32_t *>(r) >> 27) & 7u;
                        if (st == 7u) st = RXG_STATE_NONE;
                    } else {
                        st = (*reinterpret_cast<const uint32_t *>(r + 8) >> 8) & 0xFFu;
                    }
                }
                rxg_flow_sum o;
                o.tcb_idx = (int32_t)tcb;
                o.frames = v.frames;
                o.max_seq = v.max_seq;
                o.max_ack = v.max_ack;
                o.first_idx = fi;
                o.last_idx = v.last_enc - 1u;
                o.data_frames = v.data_frames;
                o.tcp_flags_or = (uint8_t)v.flags_or;
                o.state = (uint8_t)st;
                o.reserved = 0;
                o.data_bytes = v.data_bytes;
                a.out[rank] = o;
            }
            FlowSumAcc z;
            z.frames = z.max_seq = z.max_ack = z.first_enc = z.last_enc = z.data_frames = z.flags_or = z.pad = 0u;
            z.data_bytes = 0ull;
            *e = z;
        }
        if (w != 0u) *wp = 0u;
    }
}

inline uint32_t fs_tiles(uint32_t ntcb) { return (ntcb + kFsTileTcbs - 1u) / kFsTileTcbs; }

}  // namespace

size_t flow_sum_bytes(uint32_t ntcb) { return (size_t)ntcb * sizeof(FlowSumAcc); }

// (whole tiles: the count and expand passes read a tile's 64 words unconditionally)
size_t flow_sum_bits_bytes(uint32_t ntcb)
{
    return 2u * sizeof(unsigned long long) + (size_t)fs_tiles(ntcb) * kFsTileWords * sizeof(uint32_t);
}

size_t flow_sum_tile_bytes(uint32_t ntcb) { return (size_t)fs_tiles(ntcb) * sizeof(uint32_t); }

hipError_t launch_flow_sum(const LaunchFlowSum &F, hipStream_t st)
{
    if (F.n == 0) return hipMemsetAsync(F.count, 0, 3 * sizeof(unsigned long long), st);
    FsArgs a;
    a.src = F.src;
    a.recs = F.recs;
    a.acc = F.acc;
    a.left = reinterpret_cast<unsigned long long *>(F.bits);
    a.bits = F.bits + 4;
    a.tiles = F.tiles;
    a.out = F.out;
    a.cap = F.cap;
    a.count = F.count;
    a.n = F.n;
    a.nslices = (uint32_t)(((uint64_t)F.n + 63u) / 64u);
    a.rec_kind = F.rec_kind;
    a.ntcb = F.ntcb;
    a.flags = F.flags;
    a.ntiles = fs_tiles(F.ntcb);
    uint32_t ablocks = (a.nslices + 3u) / 4u;
    if (F.acc_blocks && ablocks > F.acc_blocks) ablocks = F.acc_blocks;
    if (F.max_blocks && ablocks > F.max_blocks) ablocks = F.max_blocks;
    uint32_t tblocks = (a.ntiles + 3u) / 4u;
    if (F.max_blocks && tblocks > F.max_blocks) tblocks = F.max_blocks;
    hipLaunchKernelGGL(flow_sum_acc, dim3(ablocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(flow_sum_count, dim3(tblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(flow_sum_scan, dim3(1), dim3(kFsScanLanes), 0, st, a.tiles, a.ntiles, a.left, a.count);
    hipLaunchKernelGGL(flow_sum_expand, dim3(tblocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace rxg
