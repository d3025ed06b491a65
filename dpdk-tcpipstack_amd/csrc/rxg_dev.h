// rxg_dev.h — the device primitives the burst kernels share (device code only): 16-byte
// non-temporal access, cross-lane reads, byte masks, checksum sums, the wave and workgroup
// steps of a prefix scan, a frame's slot and a record's verdict.  Every function is
// __forceinline__: a kernel that uses one compiles to what it would with the body written out.
// A new burst operation starts from these.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "rxg_common.h"
#include "rxg_kernels.h"

namespace rxg {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------- non-temporal loads and stores ---
__device__ __forceinline__ uint4 ld16(const uint8_t *p)
{
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ uint32_t ld4(const uint8_t *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(p));
}

__device__ __forceinline__ void st16(uint8_t *p, uint4 o)
{
    u32x4 v;
    v.x = o.x; v.y = o.y; v.z = o.z; v.w = o.w;
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(p));
}

// -------------------------------------------------------------------- cross-lane ---
// v of lane src_lane (0 .. 63), whatever that lane's exec bit
__device__ __forceinline__ uint32_t lane_read(uint32_t v, int src_lane)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

__device__ __forceinline__ unsigned long long lane_read64(unsigned long long v, int src_lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(uint32_t)(v >> 32));
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

__device__ __forceinline__ uint4 bperm16(uint4 v, int src_lane)
{
    uint4 r;
    r.x = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v.x);
    r.y = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v.y);
    r.z = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v.z);
    r.w = (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v.w);
    return r;
}

// lane l <- lane l + K of the same row of 16 lanes (0 past the row's end)
template <int K>
__device__ __forceinline__ uint32_t dpp_down(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + K, 0xF, 0xF, false);
}

// every lane of a group of 4 <- the group's lane Q (DPP quad_perm {Q, Q, Q, Q})
template <int Q>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, Q * 0x55, 0xF, 0xF, false);
}

// Sum of a group of LPF lanes (aligned at a multiple of LPF), valid in the group's first lane.
template <int LPF>
__device__ __forceinline__ uint32_t group_sum(uint32_t t, int lane)
{
    if constexpr (LPF >= 2) t += dpp_down<1>(t);
    if constexpr (LPF >= 4) t += dpp_down<2>(t);
    if constexpr (LPF >= 8) t += dpp_down<4>(t);
    if constexpr (LPF >= 16) t += dpp_down<8>(t);
    if constexpr (LPF >= 64) t += lane_read(t, (lane + 32) & 63);  // rows 0+2, 1+3
    if constexpr (LPF >= 32) t += lane_read(t, (lane + 16) & 63);
    return t;
}

// ------------------------------------------------------------- bytes and sums ---
// the low nb bytes of v kept (nb <= 0: none, nb >= 4: all) / dropped
__device__ __forceinline__ uint32_t keep_bytes(uint32_t v, int nb)
{
    return nb >= 4 ? v : nb <= 0 ? 0u : (v & ((1u << (8 * nb)) - 1u));
}

__device__ __forceinline__ uint32_t drop_bytes(uint32_t v, int nb)
{
    return nb >= 4 ? 0u : nb <= 0 ? v : (v & ~((1u << (8 * nb)) - 1u));
}

// acc + lo16(x) + hi16(x): one v_dot2_u32_u16 (rxg_rx_frames.h has the form with a weight)
__device__ __forceinline__ uint32_t dsum(uint32_t x, uint32_t acc)
{
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, x), __builtin_bit_cast(u16x2, 0x00010001u), acc, false);
}

// bytes [sh, sh + 16) of the 32-byte string lo || hi
__device__ __forceinline__ uint4 funnel16(uint4 lo, uint4 hi, uint32_t sh)
{
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t ds = sh >> 2, bs = sh & 3u;
    uint32_t s[5];
#pragma unroll
    for (int t = 0; t < 5; ++t)
        s[t] = ds == 0 ? w[t] : ds == 1 ? w[t + 1] : ds == 2 ? w[t + 2] : w[t + 3];
    uint4 r;
    r.x = __builtin_amdgcn_alignbyte(s[1], s[0], bs);
    r.y = __builtin_amdgcn_alignbyte(s[2], s[1], bs);
    r.z = __builtin_amdgcn_alignbyte(s[3], s[2], bs);
    r.w = __builtin_amdgcn_alignbyte(s[4], s[3], bs);
    return r;
}

// ----------------------------------------------------------------- prefix scans ---
// Inclusive scan over the wave's 64 lanes (lane = the caller's lane id); T of 4 or 8 bytes.
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v, uint32_t lane)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "a 32- or 64-bit sum");
    auto read = [](T x, int from) -> T {
        if constexpr (sizeof(T) == 8) return (T)lane_read64((unsigned long long)x, from);
        else return (T)lane_read((uint32_t)x, from);
    };
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = read(v, (int)((lane - (uint32_t)d) & 63u));
        if (lane >= (uint32_t)d) v += up;
    }
    return v;
}

// The workgroup step of a prefix scan, every lane of a workgroup of LANES lanes calling it
// with its value: `inc` the lane's inclusive sum within its wave, `before` the sum of the
// waves before the lane's, `total` the workgroup's.  wsum is the workgroup's __shared__ row;
// both barriers are inside, so the row may be used again as soon as the call returns.
template <typename T>
struct BlockScan {
    T inc, before, total;
};

template <typename T, uint32_t LANES>
__device__ __forceinline__ BlockScan<T> block_scan(T v, T (&wsum)[LANES / 64])
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    BlockScan<T> r;
    r.inc = wave_incl_scan(v, lane);
    if (lane == 63u) wsum[wave] = r.inc;
    __syncthreads();
    r.before = 0;
    r.total = 0;
#pragma unroll
    for (uint32_t w = 0; w < LANES / 64u; ++w) {
        const T x = wsum[w];
        if (w < wave) r.before += x;
        r.total += x;
    }
    __syncthreads();  // wsum is rewritten by the caller's next round
    return r;
}

// ----------------------------------------------------------- frames and records ---
// The 64-byte slot of frame i: off64[i], or with off64 null slot0 + i * stride64.
__device__ __forceinline__ uint32_t frame_slot(const uint32_t *off64, uint32_t slot0, uint32_t stride64, uint32_t i)
{
    return off64 ? off64[i] : slot0 + i * stride64;
}

__device__ __forceinline__ uint32_t frame_slot(const FrameSrc &f, uint32_t i)
{
    return frame_slot(f.off64, f.slot0, f.stride64, i);
}

// A record's fields from its words as loaded: rxg_rec8 {w0, w1}, rxg_rec16 and the first 16
// bytes of rxg_rec48 {tcb_idx, checksums, verdict | state << 8 | tcp_flags << 16 | flags << 24,
// datalen}.
__device__ __forceinline__ uint32_t rec8_verdict(uint32_t w0) { return (w0 >> 24) & 7u; }
__device__ __forceinline__ uint32_t rec16_verdict(uint32_t w2) { return w2 & 0xFFu; }

struct RecFields {
    int32_t tcb_idx;
    uint32_t verdict, tcp_flags, flags;
    int32_t datalen;
};

__device__ __forceinline__ RecFields rec8_fields(uint2 w)
{
    RecFields f;
    f.tcb_idx = (int32_t)(w.x & 0xFFFFFFu) - 1;
    f.verdict = rec8_verdict(w.x);
    f.tcp_flags = w.y & 0xFFu;
    f.flags = (w.y >> 8) & 0x3Fu;
    f.datalen = (int32_t)((w.y >> 14) & 0x1FFFFu) - 128;
    return f;
}

__device__ __forceinline__ RecFields rec16_fields(uint4 w)
{
    RecFields f;
    f.tcb_idx = (int32_t)w.x;
    f.verdict = rec16_verdict(w.z);
    f.tcp_flags = (w.z >> 16) & 0xFFu;
    f.flags = w.z >> 24;
    f.datalen = (int32_t)w.w;
    return f;
}

// The verdict in frame i's record, loaded as one dword: rxg_rec8 w0 bits 24-26, rxg_rec16 /
// rxg_rec48 byte 8.
__device__ __forceinline__ uint32_t rec_verdict(const uint8_t *recs, uint32_t rec_kind, uint32_t i)
{
    const uint8_t *r = recs + (size_t)i * rec_kind;
    return rec_kind == RXG_REC8 ? rec8_verdict(*reinterpret_cast<const uint32_t *>(r))
                                : rec16_verdict(*reinterpret_cast<const uint32_t *>(r + 8));
}

}  // namespace rxg
#endif  // __HIPCC__
