// rxg_ackplan.hip — a burst's ACKs planned per flow on the device (rxg_ack_plan_dev; the rule is
// stated in rxg.h, its host form is rxg_ackplan.cpp).
//
// Three launches on the stream, §5.11's sizes / scan / place shape.  No workgroup waits on
// another, there is no ticket and no look-back; every position is a prefix sum of the arguments,
// so the grid changes nothing.  The grids are sized from min(n, cap_trains) (the host does not
// read train_count); a workgroup whose tile lies past T' has nothing to do.
//   ak_count   a lane per train: is it its flow's first (train k - 1 has another tcb_idx), and
//              is the flow out of range, not LIVE, or does it get an ACK; per tile of kAkTile
//              trains the three sums, one 16-byte store
//   ak_scan    one workgroup: the tiles' ACK sums -> exclusive prefix sums in place, kAkScanLanes
//              a round with a carry between rounds; count[0..2] are the totals, count[3] = 0
//   ak_emit    the same decision again, ranked inside the tile on top of the tile's base: ACK a.
//              One 16-byte load of the state, for an advancing timestamp flow the order ->
//              rxopts lookup, then segs[a] as two 16-byte stores, acks[a] as one and the
//              option block as three.  The tile's ACKs that lost their block are summed over
//              the workgroup and added to count[3] by one lane (it decides no position).
//
// Roofline: launches.  Algorithmic bytes = per train 2 x 8 (tcb_idx and its neighbour's, flags
// and next_ack; twice: count and emit), per flow 2 x 16 (state), per ACK 32 + 16 written, per
// timestamp ACK 4 (order) + 16 (rxopts) read and 48 written, per tile 16 written and 2 x 16 read.
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

typedef unsigned long long u64;

struct AkArgs {
    const uint32_t *order;
    const rxg_flow_train *trains;
    const u64 *tcount;
    const uint8_t *rxopts;   // n rxg_rx_opt records or nullptr
    const uint8_t *state;    // ntcb rxg_ack_state entries
    uint8_t *opts, *segs, *acks;
    u64 *count;
    uint4 *tsum;             // ttiles entries, those of tiles below T' written {ACKs (after the scan: ACKs before the tile), not LIVE, out of range, 0}
    u64 cap;
    uint32_t n, ntcb;
    uint32_t max_trains, max_segs;  // min(n, cap_trains), min(n, cap_seg): T' and S' never exceed them
    uint32_t ttiles;
    uint32_t tsval_be;       // tsval_now as the wire holds it
    uint32_t ip_id0, opt_plain, opt_base, opt_cap;
};

// S' and T' (rxg.h): min(count, cap, n)
__device__ __forceinline__ void ak_bounds(const AkArgs &a, uint32_t *S, uint32_t *T)
{
    const u64 c0 = a.tcount[0], c1 = a.tcount[1];
    const u64 s = c0 < a.max_segs ? c0 : a.max_segs, t = c1 < a.max_trains ? c1 : a.max_trains;
    *S = (uint32_t)s;
    *T = s ? (uint32_t)t : 0u;
}

enum : uint32_t { kAkNone = 0u, kAkAck = 1u, kAkNotLive = 2u, kAkRange = 3u };

// What train k < T means for its flow: nothing (not the flow's first train), or the flow's
// class; for kAkAck *st is the flow's state as loaded {snd_nxt, rcv_ack, ts_recent, win_raw |
// flags << 16}.  The state is read only once 0 <= tcb_idx < ntcb is established.
__device__ __forceinline__ uint32_t ak_class(const AkArgs &a, uint32_t k, int32_t *tcb, uint4 *st)
{
    const int32_t me = a.trains[k].tcb_idx;
    *tcb = me;
    if (k && a.trains[k - 1u].tcb_idx == me) return kAkNone;
    if (me < 0 || (uint32_t)me >= a.ntcb) return kAkRange;
    *st = *reinterpret_cast<const uint4 *>(a.state + (size_t)me * 16u);
    return ((st->w >> 16) & RXG_AS_LIVE) ? kAkAck : kAkNotLive;
}

__global__ __launch_bounds__(kAkTile) void ak_count(AkArgs a)
{
    __shared__ uint32_t wsum[kAkTile / 64];
    uint32_t S, T;
    ak_bounds(a, &S, &T);
    for (uint32_t t = blockIdx.x; t < a.ttiles; t += gridDim.x) {
        const uint32_t k0 = t * kAkTile;
        if (k0 >= T) continue;  // (uniform over the workgroup; ak_scan and ak_emit read no tile past T')
        const uint32_t k = k0 + threadIdx.x;
        int32_t tcb;
        uint4 st;
        const uint32_t c = k < T ? ak_class(a, k, &tcb, &st) : kAkNone;
        // the three classes in one scan: 10 bits each (a tile's 256 trains may all be of one class)
        const uint32_t v = c == kAkAck ? 1u : c == kAkNotLive ? 1u << 10 : c == kAkRange ? 1u << 20 : 0u;
        const BlockScan<uint32_t> b = block_scan<uint32_t, kAkTile>(v, wsum);
        if (threadIdx.x == 0u)
            a.tsum[t] = make_uint4(b.total & 0x3FFu, (b.total >> 10) & 0x3FFu, (b.total >> 20) & 0x3FFu, 0u);
    }
}

__global__ __launch_bounds__(kAkScanLanes) void ak_scan(AkArgs a)
{
    __shared__ u64 wsum[kAkScanLanes / 64];
    uint32_t S, T;
    ak_bounds(a, &S, &T);
    const uint32_t nt = (uint32_t)(((u64)T + kAkTile - 1u) / kAkTile);  // (<= ttiles)
    u64 carry = 0, notlive = 0, range = 0;
    for (uint32_t base = 0; base < nt; base += kAkScanLanes) {
        const uint32_t e = base + threadIdx.x;
        const uint4 v = e < nt ? a.tsum[e] : make_uint4(0u, 0u, 0u, 0u);
        const BlockScan<u64> b = block_scan<u64, kAkScanLanes>((u64)v.x, wsum);
        // (T' < 2^32: an exclusive prefix sum of ACKs fits the word it replaces)
        if (e < nt) a.tsum[e].x = (uint32_t)(carry + b.before + b.inc - v.x);
        carry += b.total;
        notlive += block_scan<u64, kAkScanLanes>((u64)v.y, wsum).total;
        range += block_scan<u64, kAkScanLanes>((u64)v.z, wsum).total;
    }
    if (threadIdx.x == 0u) {
        a.count[0] = carry;
        a.count[1] = notlive;
        a.count[2] = range;
        a.count[3] = 0ull;
    }
}

__global__ __launch_bounds__(kAkTile) void ak_emit(AkArgs a)
{
    __shared__ uint32_t wsum[kAkTile / 64];
    uint32_t S, T;
    ak_bounds(a, &S, &T);
    for (uint32_t t = blockIdx.x; t < a.ttiles; t += gridDim.x) {
        const uint32_t k0 = t * kAkTile;
        if (k0 >= T) continue;  // (uniform over the workgroup)
        const uint32_t k = k0 + threadIdx.x;
        int32_t tcb = 0;
        uint4 st = make_uint4(0u, 0u, 0u, 0u);
        const bool is_ack = k < T && ak_class(a, k, &tcb, &st) == kAkAck;
        const BlockScan<uint32_t> b = block_scan<uint32_t, kAkTile>(is_ack ? 1u : 0u, wsum);
        uint32_t lost = 0;
        if (is_ack) {
            const u64 rank = (u64)a.tsum[t].x + b.before + b.inc - 1u;
            const uint2 w3 = reinterpret_cast<const uint2 *>(a.trains + k)[3];  // next_ack, flags
            const bool adv = (w3.y & RXG_FTR_HEAD) != 0u;
            uint32_t fl = adv ? (uint32_t)RXG_ACK_ADVANCES | ((w3.y & RXG_FTR_FIN) ? (uint32_t)RXG_ACK_FIN : 0u)
                              : (uint32_t)RXG_ACK_DUP;
            const uint32_t ack = adv ? w3.x : st.y;
            const uint32_t sflags = st.w >> 16;
            uint32_t reserved = a.opt_plain;
            bool block = false;
            if ((sflags & RXG_AS_TS) && a.opts) {
                if ((u64)a.opt_base + rank < a.opt_cap) {
                    reserved = (uint32_t)(a.opt_base + rank + 1ull);
                    block = rank < a.cap;
                } else {
                    fl |= RXG_ACK_NO_OPT;
                    lost = 1u;
                }
            }
            if (block) {
                uint32_t tsecr = st.z;
                if (adv && a.rxopts) {
                    const uint32_t first = a.trains[k].first;
                    if (first < S) {
                        const uint32_t pkt = a.order[first];
                        if (pkt < a.n) {
                            const uint4 o = *reinterpret_cast<const uint4 *>(a.rxopts + (size_t)pkt * 16u);
                            if ((o.w >> 16) & RXG_O_TS) tsecr = o.x;
                        }
                    }
                }
                // rxg_tx_opt: len at 0, bytes[] at 6: 01 01 08 0A, TSval, TSecr big-endian, the rest zero
                const uint32_t be = __builtin_bswap32(tsecr);
                uint8_t *o = a.opts + ((size_t)a.opt_base + rank) * 48u;
                st16(o, make_uint4(12u, 0x01010000u, 0x0A08u | (a.tsval_be << 16), (a.tsval_be >> 16) | (be << 16)));
                st16(o + 16, make_uint4(be >> 16, 0u, 0u, 0u));
                st16(o + 32, make_uint4(0u, 0u, 0u, 0u));
            }
            if (rank < a.cap) {
                uint8_t *g = a.segs + (size_t)rank * 32u;
                // rxg_tx_seg: src_off 0 | flow, seq | ack, data_len 0, win_raw | ip_id, tcp_flags, pad 0 | reserved
                st16(g, make_uint4(0u, 0u, (uint32_t)tcb, st.x));
                st16(g + 16, make_uint4(ack, (st.w & 0xFFFFu) << 16,
                                        ((a.ip_id0 + (uint32_t)rank) & 0xFFFFu) | ((uint32_t)RXG_TCP_FLAG_ACK << 16),
                                        reserved));
                st16(a.acks + (size_t)rank * 16u, make_uint4((uint32_t)tcb, ack, st.x, fl | (k << 8)));
            }
        }
        const BlockScan<uint32_t> ls = block_scan<uint32_t, kAkTile>(lost, wsum);
        if (threadIdx.x == 0u && ls.total) atomicAdd(&a.count[3], (u64)ls.total);
    }
}

inline uint32_t ak_tiles(uint32_t entries) { return (uint32_t)(((uint64_t)entries + kAkTile - 1u) / kAkTile); }
inline uint32_t ak_max_trains(uint32_t n, unsigned long long cap_trains) { return cap_trains < n ? (uint32_t)cap_trains : n; }

}  // namespace

size_t ack_plan_scratch_bytes(uint32_t n, unsigned long long cap_trains)
{
    return (size_t)ak_tiles(ak_max_trains(n, cap_trains)) * sizeof(uint4);
}

int ack_plan_blocks_per_cu()
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, ak_emit, (int)kAkTile, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

hipError_t launch_ack_plan(const LaunchAckPlan &P, hipStream_t st)
{
    AkArgs a;
    a.order = P.order;
    a.trains = P.trains;
    a.tcount = P.train_count;
    a.rxopts = reinterpret_cast<const uint8_t *>(P.rxopts);
    a.state = reinterpret_cast<const uint8_t *>(P.state);
    a.opts = reinterpret_cast<uint8_t *>(P.opts);
    a.segs = reinterpret_cast<uint8_t *>(P.segs);
    a.acks = reinterpret_cast<uint8_t *>(P.acks);
    a.count = P.count;
    a.tsum = reinterpret_cast<uint4 *>(P.scratch);
    a.cap = P.cap;
    a.n = P.n;
    a.ntcb = P.ntcb;
    a.max_trains = ak_max_trains(P.n, P.cap_trains);
    a.max_segs = P.cap_seg < P.n ? (uint32_t)P.cap_seg : P.n;
    a.ttiles = ak_tiles(a.max_trains);
    a.tsval_be = __builtin_bswap32(P.tsval_now);
    a.ip_id0 = P.ip_id0;
    a.opt_plain = P.opt_plain;
    a.opt_base = P.opt_base;
    a.opt_cap = P.opt_cap;
    // no train can be read: the four words, nothing else
    if (a.ttiles == 0u || a.max_segs == 0u) return hipMemsetAsync(P.count, 0, 4 * sizeof(u64), st);
    const uint32_t cap = P.max_blocks ? P.max_blocks : 1u << 16;
    const uint32_t blocks = std::min(a.ttiles, cap);
    hipLaunchKernelGGL(ak_count, dim3(blocks), dim3(kAkTile), 0, st, a);
    hipLaunchKernelGGL(ak_scan, dim3(1), dim3(kAkScanLanes), 0, st, a);
    hipLaunchKernelGGL(ak_emit, dim3(blocks), dim3(kAkTile), 0, st, a);
    return hipGetLastError();
}

}  // namespace rxg
