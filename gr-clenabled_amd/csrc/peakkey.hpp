// The peak key: how clPulseSearch (psearch.hip), clPeriodSearch (ffa.hip) and clSpectralSearch (ssearch.hip) find and report the
// record {snr, loc} of a block.  The contract is in include/mi355_clenabled.h; this is its one implementation.
//
//     key = {order-preserving map of snr's bits, ~loc},  loc = (level << 24) | position
//
// The largest key of a block is its record with the documented ties: the largest snr, then the smallest level, then the smallest
// position.  A NaN maps to 0, below the map of every value, so it never takes part.  The maximum does not depend on the order of
// the reduction: registers (fold), a wave (wave_max, wave_min), LDS atomics and global 64-bit integer atomicMax may all take part.
// The arithmetic that produces snr stays with each block.
#pragma once
#include <cstdint>
#include <vector>
#include "common.h"

#pragma clang fp contract(off)

namespace peakkey {

typedef unsigned long long u64;

constexpr u64 kEmpty = 0x007FFFFF00000000ull;  // the key that decodes to {-Inf, 0xFFFFFFFF}: below the key of every value

// c_k: the binary32 nearest to 2^(-k/2)
__device__ __forceinline__ float c(int k) { return __uint_as_float(((k & 1) ? 0x3F3504F3u : 0x3F800000u) - ((unsigned)(k >> 1) << 23)); }

// one snr folded into the running best (ordered snr, level) of its position: ascending levels and a strict comparison keep the
// smallest level of equals.  Straight-line code (selects, no branches)
__device__ __forceinline__ void fold(float snr, int level, unsigned &best_ordered, unsigned &best_level)
{
    const unsigned u = __float_as_uint(snr);
    unsigned o = u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
    o = snr == snr ? o : 0u;
    best_level = o > best_ordered ? (unsigned)level : best_level;
    best_ordered = o > best_ordered ? o : best_ordered;
}

__device__ __forceinline__ u64 key(unsigned ordered, unsigned loc) { return ((u64)ordered << 32) | (u64)(~loc); }

// key -> {snr's bits, loc}.  ZERO_IS_EMPTY: 0, a zeroed slot that no value has reached, reads as kEmpty (k_peak_emit's keys start
// at kEmpty and leave the test out)
template <bool ZERO_IS_EMPTY = true> __device__ __forceinline__ uint2 record(u64 key)
{
    if (ZERO_IS_EMPTY && key == 0) key = kEmpty;
    const unsigned o = (unsigned)(key >> 32);
    return make_uint2((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o, ~(unsigned)key);
}

struct UMax {
    __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a > b ? a : b; }
};
struct UMin {
    __device__ __forceinline__ unsigned operator()(unsigned a, unsigned b) const { return a < b ? a : b; }
};

template <int CTRL, class Op> __device__ __forceinline__ unsigned dpp_step(unsigned v, Op op)
{
    return op(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false));
}

// op over a wave (all 64 lanes active), the same in every lane: pairs, quads, half rows and rows of 16 by DPP, the four rows
// through scalar registers
template <class Op> __device__ __forceinline__ unsigned wave_reduce(unsigned v, Op op)
{
    v = dpp_step<0xB1>(v, op);   // quad_perm:[1,0,3,2]
    v = dpp_step<0x4E>(v, op);   // quad_perm:[2,3,0,1]
    v = dpp_step<0x141>(v, op);  // row_half_mirror
    v = dpp_step<0x140>(v, op);  // row_mirror
    const unsigned r0 = (unsigned)__builtin_amdgcn_readlane((int)v, 0), r1 = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
    const unsigned r2 = (unsigned)__builtin_amdgcn_readlane((int)v, 32), r3 = (unsigned)__builtin_amdgcn_readlane((int)v, 48);
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ unsigned wave_max(unsigned v) { return wave_reduce(v, UMax()); }
__device__ __forceinline__ unsigned wave_min(unsigned v) { return wave_reduce(v, UMin()); }

namespace {  // kernels of a header that several translation units include: internal linkage

// the peaks buffer carries the keys of a call: every slot starts at kEmpty, the candidate counters at zero.  (A template, like
// k_peak_emit: a block that launches neither, clPeriodSearch, carries neither.)
template <int THREADS = 256> __global__ __launch_bounds__(THREADS) void k_peak_init(u64 *keys, long long count, unsigned *counts)
{
    const long long first = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (counts && first == 0) { counts[0] = 0; counts[1] = 0; }
    for (long long i = first; i < count; i += (long long)gridDim.x * THREADS) keys[i] = kEmpty;
}

// keys -> {float snr; uint32 loc} in place; records at or above the threshold -> {snr, loc, series, block}, counted in full.
// Split()(i, shape) -> {series, block} of record i of the peaks buffer, whose shape the block describes with one int
template <class Split>
__global__ __launch_bounds__(256) void k_peak_emit(u64 *peaks, long long count, int shape, float thr, uint2 *cands, long long max_cands,
                                                   unsigned *counts)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const uint2 r = record<false>(peaks[i]);
        peaks[i] = ((u64)r.y << 32) | r.x;
        if (cands && __uint_as_float(r.x) >= thr) {
            const unsigned at = atomicAdd(&counts[0], 1u);
            if ((long long)at < max_cands) {
                atomicAdd(&counts[1], 1u);
                cands[2 * (size_t)at] = r;
                cands[2 * (size_t)at + 1] = Split()(i, shape);
            }
        }
    }
}

}  // namespace

// ---- host side -------------------------------------------------------------------------------------------------------------------

// the cands / counts arguments of a work call: present together, aligned
inline int check_cands(const void *cands, const void *counts)
{
    if (cands) {
        MI355_REQUIRE(counts != nullptr, "cands without counts");
        MI355_REQUIRE((reinterpret_cast<uintptr_t>(cands) & 7u) == 0, "cands must be 8-byte aligned");
        MI355_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7u) == 0, "counts must be 8-byte aligned");
    }
    return MI355_OK;
}

// ... and apart from the ib bytes of in, the pb bytes of peaks and each other
inline int check_cands_apart(const void *in, long long ib, const void *peaks, long long pb, const void *cands, long long max_cands, const void *counts)
{
    if (cands) {
        const long long cb = 16 * max_cands;
        MI355_REQUIRE(max_cands == 0 || !mi355_overlap(in, ib, cands, cb), "in and cands overlap");
        MI355_REQUIRE(!mi355_overlap(in, ib, counts, 8), "in and counts overlap");
        MI355_REQUIRE(max_cands == 0 || !mi355_overlap(peaks, pb, cands, cb), "peaks and cands overlap");
        MI355_REQUIRE(!mi355_overlap(peaks, pb, counts, 8), "peaks and counts overlap");
        MI355_REQUIRE(max_cands == 0 || !mi355_overlap(cands, cb, counts, 8), "cands and counts overlap");
    }
    return MI355_OK;
}

// The candidates of a work() that runs in pieces: each piece leaves its counters {found, stored} and its list on the device; the
// lists are appended to the caller's until max_cands are stored, `found` is counted in full and saturates.
struct CandList {
    enum Field { SERIES = 2, BLOCK = 3 };  // word of the 16-byte record {snr, loc, series, block}
    uint32_t *cands;
    long long max_cands;
    unsigned long long found = 0;
    long long stored = 0;
    std::vector<uint32_t> got;

    CandList(void *cands_, long long max_cands_) : cands((uint32_t *)cands_), max_cands(max_cands_) {}

    // behind a piece's launches on st: waits for them, fetches what they found and appends it with `offset` (the piece's first
    // series or block, counted from the call's) added to `field`
    int append(const void *d_counts, const void *d_cands, Field field, long long offset, hipStream_t st)
    {
        uint32_t c[2] = {0, 0};
        MI355_HIP(hipMemcpyAsync(c, d_counts, 8, hipMemcpyDeviceToHost, st));
        MI355_HIP(hipStreamSynchronize(st));
        found += c[0];
        if (c[1]) {
            got.resize(4 * (size_t)c[1]);
            MI355_HIP(hipMemcpyAsync(got.data(), d_cands, 16 * (size_t)c[1], hipMemcpyDeviceToHost, st));
            MI355_HIP(hipStreamSynchronize(st));
            for (uint32_t i = 0; i < c[1] && stored < max_cands; i++, stored++) {
                uint32_t *dst = cands + 4 * stored;
                memcpy(dst, got.data() + 4 * (size_t)i, 16);
                dst[field] += (uint32_t)offset;
            }
        }
        return MI355_OK;
    }

    // after the last piece: the caller's counters
    void finish(void *counts) const
    {
        ((uint32_t *)counts)[0] = found > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)found;
        ((uint32_t *)counts)[1] = (uint32_t)stored;
    }
};

// The per-series statistics of a handle: the host image [mean S | inv_sigma S] and its versions on the device.  The caller holds
// the handle's lock where there is one to hold and has set the device for publish, set and release.
struct SeriesStats {
    std::vector<float> host;
    mi355_tables dev;
    size_t S = 0;
    const char *what = "";  // of a failed upload: "mi355_xxx: statistics"

    // host image only; NULL: mean 0, inv_sigma 1
    void init(size_t S_, const float *mean, const float *inv_sigma, const char *what_)
    {
        S = S_;
        what = what_;
        host.assign(2 * S, 0.0f);
        for (size_t s = 0; s < S; s++) {
            host[s] = mean ? mean[s] : 0.0f;
            host[S + s] = inv_sigma ? inv_sigma[s] : 1.0f;
        }
    }
    int publish(mi355_ctx *ctx) { return dev.publish(ctx, host.data(), 2 * S * 4, what); }
    // on failure the version in use stays, on the host and on the device
    int set(mi355_ctx *ctx, const float *mean, const float *inv_sigma)
    {
        std::vector<float> img(2 * S);
        memcpy(img.data(), mean, S * 4);
        memcpy(img.data() + S, inv_sigma, S * 4);
        const int rc = dev.publish(ctx, img.data(), 2 * S * 4, what);
        if (rc) return rc;
        host.swap(img);
        return MI355_OK;
    }
    void get(float *mean, float *inv_sigma) const
    {
        memcpy(mean, host.data(), S * 4);
        memcpy(inv_sigma, host.data() + S, S * 4);
    }
    const float *current() const { return (const float *)dev.current(); }
    int used(hipStream_t st) { return dev.used(st); }  // this version may be released behind the launches that st holds so far
    void release() { dev.release(); }
};

}  // namespace peakkey
