// rxg_rxopt.hip — the TCP options of a burst's segments parsed on the device from its frames
// and records (rxg_rx_opts_dev; the rule is stated in rxg.h, its host form is rxg_rxopt.cpp).
//
// One launch, no workgroup waits on another, no buffer of the context.  A wave takes a
// 64-frame slice (grid-stride); lane i owns frame i of the slice:
//   - it reads its record's verdict, len[i] and its offset;
//   - a candidate (DISPATCH / RST_NOPCB / RST_LISTEN_NONSYN) loads, non-temporal and
//     together, the dword at frame byte 44 (data_off is its byte 2) and the 16-byte chunks 3
//     and 4 (frame bytes 48-79: option bytes 0-25, every timestamp segment and a typical
//     SYN).  A load is issued only when the frame has a byte in it that the parse uses, so
//     it stays inside the 64-byte line of the frame's last byte: a 60-byte frame that claims
//     40 option bytes loads nothing of the next line.  Chunk 5 (bytes 80-95) is loaded only
//     by the lanes with O > 26 and len > 80, under a wave-uniform test: the one dependent
//     round trip, paid by slices that hold such a frame;
//   - bytes at and beyond len[i] are zeroed, the 40 option bytes are shifted into ten
//     dwords (frame byte 54 is byte 2 of a dword: v_alignbyte);
//   - O == 0, or O == 12 with option dword 0 equal to 01 01 08 0A (RFC 7323 appendix A, what
//     rxg_tx_opt_timestamp builds), is answered with one compare and two byte swaps; when
//     every candidate of the slice is of that kind the wave skips the walk;
//   - the others take the walk, one option per round until the slice's last walking lane is
//     done: a lane brings the ten bytes at its own position p (kind, length, the longest
//     value read) to three dwords by picking four of the ten with select chains and
//     v_alignbyte, so no array is indexed by a lane's value (no scratch, no LDS);
//   - every lane stores its record with one 16-byte non-temporal store: a wave writes 1 KiB
//     contiguous.  Other frames' records are zero.
//
// Roofline: HBM, algorithmic bytes = n * record size + 6 n (off64 + len; 2 n in strided
// mode) + per candidate the 64-byte lines that hold bytes 32 .. 54 + O and lie inside the
// frame (64 or 128) + 16 n written.
#include "rxg_dev.h"
#include "rxg_kernels.h"

namespace rxg {
namespace {

struct RoArgs {
    FrameSrc src;
    const uint8_t *recs;
    uint8_t *out;
    uint32_t n, nslices, rec_kind;
};

__device__ __forceinline__ bool is_candidate(const RoArgs &a, uint32_t i)
{
    return rec_verdict(a.recs, a.rec_kind, i) <= RXG_V_RST_LISTEN_NONSYN;
}

// The option bytes as eleven dwords: b[j] is byte j & 3 of o[j >> 2], o[10] is zero.
constexpr int kOptDwords = 11;

// o[m] for a lane's own m (0 past the array), picked from registers by a chain of selects:
// an array indexed by a lane's value would live in scratch.
__device__ __forceinline__ uint32_t pick(const uint32_t (&o)[kOptDwords], uint32_t m)
{
    uint32_t v = 0u;
#pragma unroll
    for (int j = 0; j < kOptDwords; ++j) v = m == (uint32_t)j ? o[j] : v;
    return v;
}

struct Found {
    uint32_t tsval, tsecr, mss, wscale, nsack, sack_off, flags;
};

constexpr uint32_t kAlignedTs = 0x0A080101u;  // 01 01 08 0A as a little-endian dword

// One step of the walk of rxg.h for a lane whose walk stands at p < O: the ten bytes
// b[p .. p + 10) -- kind, length and the longest value the rule reads (a timestamp's) --
// are brought to three dwords, the option is taken, p moves on or the walk ends.
__device__ __forceinline__ void walk_step(const uint32_t (&o)[kOptDwords], uint32_t O, uint32_t &p, bool &live,
                                          Found &r)
{
    const uint32_t m = p >> 2, sh = p & 3u;
    const uint32_t r0 = pick(o, m), r1 = pick(o, m + 1u), r2 = pick(o, m + 2u), r3 = pick(o, m + 3u);
    const uint32_t w0 = __builtin_amdgcn_alignbyte(r1, r0, sh), w1 = __builtin_amdgcn_alignbyte(r2, r1, sh),
                   w2 = __builtin_amdgcn_alignbyte(r3, r2, sh);
    const uint32_t k = w0 & 0xFFu, l = (w0 >> 8) & 0xFFu;
    const uint32_t v0 = __builtin_bswap32((w0 >> 16) | (w1 << 16));  // b[p+2 .. p+6), big-endian
    const uint32_t v1 = __builtin_bswap32((w1 >> 16) | (w2 << 16));  // b[p+6 .. p+10)
    // (selects, not branches that assign to fields: those would put `r` into scratch)
    const bool eol = k == 0u, nop = k == 1u;
    const bool bad = !eol && !nop && (p + 1u >= O || l < 2u || p + l > O);
    const bool opt = !eol && !nop && !bad;
    const bool mss = opt && k == 2u && l == 4u, ws = opt && k == 3u && l == 3u, sp = opt && k == 4u && l == 2u;
    const bool sack = opt && k == 5u && (l == 10u || l == 18u || l == 26u || l == 34u);
    const bool ts = opt && k == 8u && l == 10u;
    r.mss = mss ? v0 >> 16 : r.mss;
    r.wscale = ws ? v0 >> 24 : r.wscale;
    r.nsack = sack ? (l - 2u) >> 3 : r.nsack;
    r.sack_off = sack ? 54u + p + 2u : r.sack_off;
    r.tsval = ts ? v0 : r.tsval;
    r.tsecr = ts ? v1 : r.tsecr;
    r.flags |= (bad ? RXG_O_MALFORMED : 0u) | (mss ? RXG_O_MSS : 0u) | (ws ? RXG_O_WSCALE : 0u) |
               (sp ? RXG_O_SACK_PERM : 0u) | (sack ? RXG_O_SACK : 0u) | (ts ? RXG_O_TS : 0u) |
               (opt && !(mss || ws || sp || sack || ts) ? RXG_O_OTHER : 0u);
    p += nop ? 1u : opt ? l : 0u;
    live = !eol && !bad && p < O;
}

__global__ __launch_bounds__(256) void rx_opts_parse(RoArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    for (uint32_t s = wave; s < a.nslices; s += nwaves) {
        const uint32_t i = s * 64u + lane;
        const bool in = i < a.n;
        const bool cand = in && is_candidate(a, i);
        uint32_t ln = 0;
        const uint8_t *f = a.src.frames;
        if (cand) {
            const uint32_t off = frame_slot(a.src, i);
            ln = a.src.len[i];
            f = a.src.frames + (size_t)off * 64u;  // 64-bit: a pool may pass 4 GiB
        }
        // every load below lies in a line that holds a frame byte below len
        uint32_t w44 = 0;
        uint4 c3 = make_uint4(0u, 0u, 0u, 0u), c4 = c3, c5 = c3;
        if (cand && ln > 46u) w44 = ld4(f + 44);
        if (cand && ln > 54u) c3 = ld16(f + 48);
        if (cand && ln > 64u) c4 = ld16(f + 64);
        const uint32_t d = (w44 >> 20) & 0xFu;  // frame[46] >> 4
        const uint32_t O = d < 5u ? 0u : 4u * d - 20u;
        const bool far = cand && O > 26u && ln > 80u;
        if (__ballot(far) != 0ull) {
            if (far) c5 = ld16(f + 80);
        }
        // bytes at and beyond len read as zero (frame bytes 52 .. 95)
        uint32_t sw[kOptDwords] = {c3.y, c3.z, c3.w, c4.x, c4.y, c4.z, c4.w, c5.x, c5.y, c5.z, c5.w};
        if (ln < 96u) {
#pragma unroll
            for (int m = 0; m < kOptDwords; ++m) sw[m] = keep_bytes(sw[m], (int)ln - (52 + 4 * m));
        }
        uint32_t o[kOptDwords];
#pragma unroll
        for (int m = 0; m < kOptDwords - 1; ++m) o[m] = __builtin_amdgcn_alignbyte(sw[m + 1], sw[m], 2u);
        o[kOptDwords - 1] = 0u;

        Found r = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
        if (cand) r.flags = RXG_O_PARSED | (d < 5u ? RXG_O_BAD_DOFF : 0u) | (54u + O > ln ? RXG_O_CUT : 0u);
        const bool aligned = cand && O == 12u && o[0] == kAlignedTs;
        if (aligned) {
            r.tsval = __builtin_bswap32(o[1]);
            r.tsecr = __builtin_bswap32(o[2]);
            r.flags |= RXG_O_TS;
        }
        bool live = cand && O != 0u && !aligned;
        uint32_t p = 0;
        while (__ballot(live) != 0ull) {
            if (live) walk_step(o, O, p, live, r);
        }
        if (in) {
            // rxg_rx_opt: tsval, tsecr, {mss, wscale, nsack}, {sack_off, opt_len, flags}
            const uint4 rec = make_uint4(r.tsval, r.tsecr, r.mss | (r.wscale << 16) | (r.nsack << 24),
                                         r.sack_off | ((cand ? O : 0u) << 8) | (r.flags << 16));
            st16(a.out + (size_t)i * 16u, rec);
        }
    }
}

}  // namespace

int rx_opts_blocks_per_cu()
{
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, rx_opts_parse, 256, 0);
    return (e == hipSuccess && n > 0) ? n : 4;
}

hipError_t launch_rx_opts(const LaunchRxOpts &R, hipStream_t st)
{
    if (R.n == 0) return hipSuccess;
    const RoArgs a = {R.src, R.recs, R.out, R.n, (uint32_t)(((uint64_t)R.n + 63u) / 64u), R.rec_kind};
    uint32_t blocks = (a.nslices + 3u) / 4u;
    if (R.max_blocks && blocks > R.max_blocks) blocks = R.max_blocks;
    hipLaunchKernelGGL(rx_opts_parse, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace rxg
