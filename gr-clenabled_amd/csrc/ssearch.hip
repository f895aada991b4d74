// clSpectralSearch: FFT periodicity search with exact incoherent harmonic sums over the S dedispersed time series that clDedisperser
// delivers, as gfx950 HIP kernels.  The contract is in include/mi355_clenabled.h; the reference module has no such block.
//
//   spectrum stage (SERIES input, floating point, held to a derived bound)
//     z[n] = x[2n] + i x[2n+1], Z = FFT_Nb(z) by an internal clFFT handle, then per bin k < Nb = N / 2
//     X[k] = (Z[k] + conj Z[Nb-k]) / 2 - i e^(-2 pi i k / N) (Z[k] - conj Z[Nb-k]) / 2;   w[k] = |X[k]|^2 inv_sigma^2 / N,  +0 below k_lo
//   harmonic-sum stage (the contract, bit for bit)
//     s_0[k] = w[k];  s_h[k] = ((s_(h-1)[k] + w[r(k,1,h)]) + w[r(k,3,h)]) + ... + w[r(k,2^h-1,h)],  r(k,j,h) = (k j + 2^(h-1)) >> h
//     snr_h[k] = (s_h[k] - 2^h) c_h;   record of (series, block of Bb bins) = the largest 64-bit key {map of snr's bits, ~((h << 24) | k)}
//
// k_ss_pack   series at a pitch other than N (or an input the transform cannot take as it lies) -> rows of N floats in scratch
// k_ss_power  untangles the half-length transform and detects in one pass over Z: a thread owns the pair (k, Nb - k), which share
//             their two Z values and, up to signs, their twiddle (table of Nb / 2 + 1 entries made in double on the host)
// k_ss_tiled  the default route.  A workgroup owns (series, tile of Tk bins); a thread owns bins tid + 256 i and keeps their running
//             sums in registers across the levels.  Level h: for every odd j the contiguous window w[r(k0,j,h) .. r(k0+Tk-1,j,h)] is
//             staged in LDS (16-byte loads where the address allows, 4-byte ones at the ragged ends: `in` may sit at any 4-byte
//             alignment and nothing outside the window is read), then every bin adds its operand of each window, odd j ascending.
//             Neighbouring lanes read the same or the adjacent word.  The keys of a wave are reduced with DPP, a tile's in LDS, a
//             block's (Bb > Tk) with one 64-bit integer atomicMax per tile into the peaks buffer itself.
// k_ss_gen    the generic route: one thread per bin gathers from global memory.
// The key and its kernels (k_peak_init, k_peak_emit) are peakkey.hpp's, as clPulseSearch: the peaks buffer carries the keys of a
// call and is decoded in place; candidates by an integer counter.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"
#include "peakkey.hpp"

#pragma clang fp contract(off)

namespace {

using peakkey::u64;

constexpr int kSsMaxS = 1 << 20, kSsMinLog2N = 8, kSsMaxLog2N = 22, kSsMaxH = 5, kSsMinBb = 16;
constexpr long long kSsMaxBytes = 1ll << 40;
constexpr long long kSsHostBytes = 4ll << 20;     // host path: input bytes per staged piece unless one series needs more
constexpr long long kSsChunkFloats = 1ll << 24;   // SERIES input: series share a chunk while its samples stay below this (64 MiB)
constexpr int kSsThreads = 256, kSsEp = 4;        // a tile holds at most 256 x 4 bins
constexpr int kSsMaxTk = kSsThreads * kSsEp;
// LDS of a level: its 2^(h-1) windows hold at most Tk 2^(h-2) + 2^h floats, and each is placed 0 .. 3 floats into a slot rounded up
// to a multiple of 4: 8 Tk + 32 + 16 x 6 at h = 5
constexpr int kSsLdsFloats = 8 * kSsMaxTk + 32 + 96;

// snr_h of one sum folded into the running best of its bin
__device__ __forceinline__ void ss_fold(float sum, int h, unsigned &bo, unsigned &bh)
{
    const float d = sum - (float)(1 << h);
    peakkey::fold(d * peakkey::c(h), h, bo, bh);
}

__device__ __forceinline__ unsigned ss_r(unsigned k, unsigned j, int h) { return (k * j + (1u << (h - 1))) >> h; }  // k j < 2^26

// rows of n2 float2 at pitch in_pitch floats -> rows of n2 float2
__global__ __launch_bounds__(256) void k_ss_pack(const float2 *__restrict__ in, long long in_pitch2, float2 *__restrict__ out, long long total, int log2_n2)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long s = i >> log2_n2, t = i & ((1ll << log2_n2) - 1);
        out[i] = in[(size_t)s * (size_t)in_pitch2 + (size_t)t];
    }
}

// one bin from its two half-length bins a = Z[k], b = Z[Nb - k] and (c, s) = (cos, sin)(2 pi k / N)
__device__ __forceinline__ float ss_bin(float2 a, float2 b, float c, float s, float g)
{
    const float er = 0.5f * (a.x + b.x), ei = 0.5f * (a.y - b.y);  // (Z[k] + conj Z[Nb-k]) / 2
    const float dr = 0.5f * (a.x - b.x), di = 0.5f * (a.y + b.y);  // (Z[k] - conj Z[Nb-k]) / 2
    const float xr = er + (c * di - s * dr);
    const float xi = ei - (c * dr + s * di);
    return (xr * xr + xi * xi) * g;
}

// Z: nS rows of Nb float2; tw: Nb / 2 + 1 entries (cos, sin)(2 pi k / N); isg: inv_sigma of the launch's first series;
// w: nS rows of Nb floats.  Item (s, t), t < Nb / 2: bins t and Nb - t; t = 0: bins 0 and Nb / 2, each its own partner
__global__ __launch_bounds__(256) void k_ss_power(const float2 *__restrict__ Z, const float2 *__restrict__ tw, const float *__restrict__ isg,
                                                  float *__restrict__ w, long long total, int log2_nb, int k_lo, float inv_n)
{
    const int Nb = 1 << log2_nb, half = Nb >> 1;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long s = i >> (log2_nb - 1);
        const int t = (int)(i & (half - 1));
        const float2 *z = Z + (size_t)s * (size_t)Nb;
        float *y = w + (size_t)s * (size_t)Nb;
        const float q = isg[s];
        const float g = (q * q) * inv_n;
        const int k2 = t ? Nb - t : half;
        const float2 a = z[t], b = z[k2];
        const float2 c1 = tw[t];
        float w1, w2;
        if (t) {
            w1 = ss_bin(a, b, c1.x, c1.y, g);
            w2 = ss_bin(b, a, -c1.x, c1.y, g);
        } else {
            const float2 c2 = tw[half];
            w1 = ss_bin(a, a, c1.x, c1.y, g);
            w2 = ss_bin(b, b, c2.x, c2.y, g);
        }
        y[t] = t < k_lo ? 0.0f : w1;
        y[k2] = k2 < k_lo ? 0.0f : w2;
    }
}

struct SsArgs {
    int H, log2_nb, log2_bb, log2_tk;
    long long in_pitch;
    long long units;  // series of the launch x tiles per series
};

// keys: the call's peaks buffer at the launch's first series, [series][block] 64-bit keys (k_peak_init has filled it)
__global__ __launch_bounds__(kSsThreads) void k_ss_tiled(const float *__restrict__ in, u64 *keys, const SsArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[kSsLdsFloats];
    __shared__ u64 lkeys[kSsMaxTk / kSsMinBb];
    const int tid = threadIdx.x, lane = tid & 63;
    const int Tk = 1 << a.log2_tk;
    const int tiles_log2 = a.log2_nb - a.log2_tk;
    const int nbl = a.log2_tk > a.log2_bb ? 1 << (a.log2_tk - a.log2_bb) : 1;  // blocks a tile touches
    const unsigned bmask = (1u << a.log2_bb) - 1;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const long long s = u >> tiles_log2;
        const unsigned k0 = (unsigned)(u & ((1ll << tiles_log2) - 1)) << a.log2_tk;
        const float *x = in + (size_t)s * (size_t)a.in_pitch;
        if (tid < nbl) lkeys[tid] = 0;
        float acc[kSsEp];
        unsigned bo[kSsEp], bh[kSsEp];
#pragma unroll
        for (int e = 0; e < kSsEp; e++) {
            const int p = tid + kSsThreads * e;
            acc[e] = x[k0 + (p < Tk ? p : 0)];
            bo[e] = 0;
            bh[e] = 0;
            ss_fold(acc[e], 0, bo[e], bh[e]);
        }
        for (int h = 1; h <= a.H; h++) {
            // stage the level's windows behind one another; window of j: floats [wa, wb] of the series, placed (address of wa in
            // floats) & 3 floats into its slot, so that the 16-byte loads and the 16-byte LDS stores are both aligned
            unsigned slot = 0;
            for (unsigned j = 1; j < (1u << h); j += 2) {
                const unsigned wa = ss_r(k0, j, h), wb = ss_r(k0 + (unsigned)Tk - 1, j, h), len = wb - wa + 1;
                const float *src = x + wa;
                const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
                const unsigned head = (4u - mis) & 3u;  // floats before the first aligned one
                float *dst = lds + slot + mis;
                if (len <= head) {
                    if ((unsigned)tid < len) dst[tid] = src[tid];
                } else {
                    const unsigned nq = (len - head) >> 2, tail0 = head + 4 * nq;
                    if ((unsigned)tid < head) dst[tid] = src[tid];
                    if ((unsigned)tid < len - tail0) dst[tail0 + tid] = src[tail0 + tid];
                    const float4 *src4 = reinterpret_cast<const float4 *>(src + head);
                    float4 *dst4 = reinterpret_cast<float4 *>(dst + head);
                    for (unsigned q = tid; q < nq; q += kSsThreads) dst4[q] = src4[q];
                }
                slot += (mis + len + 3u) & ~3u;
            }
            __syncthreads();
            slot = 0;
            for (unsigned j = 1; j < (1u << h); j += 2) {
                const unsigned wa = ss_r(k0, j, h), wb = ss_r(k0 + (unsigned)Tk - 1, j, h), len = wb - wa + 1;
                const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(x + wa) >> 2) & 3u);
                const float *win = lds + slot + mis;
#pragma unroll
                for (int e = 0; e < kSsEp; e++) {
                    const int p = tid + kSsThreads * e;
                    const unsigned k = k0 + (unsigned)(p < Tk ? p : 0);
                    acc[e] = acc[e] + win[ss_r(k, j, h) - wa];
                }
                slot += (mis + len + 3u) & ~3u;
            }
#pragma unroll
            for (int e = 0; e < kSsEp; e++) ss_fold(acc[e], h, bo[e], bh[e]);
            __syncthreads();  // the windows are free for the next level
        }
        __syncthreads();  // lkeys is zero for every wave (with H = 0 no level's barrier lies between the store above and the atomics below)
        // a wave holds 64 consecutive bins of the tile
#pragma unroll
        for (int e = 0; e < kSsEp; e++) {
            const int p = tid + kSsThreads * e;
            const unsigned k = k0 + (unsigned)p;
            const unsigned o = p < Tk ? bo[e] : 0u;  // 0: nothing to report
            const unsigned bl = a.log2_tk > a.log2_bb ? (unsigned)p >> a.log2_bb : 0u;
            const unsigned loc = (bh[e] << 24) | (k & bmask);
            const u64 live = __ballot(o != 0);
            if (live) {  // (uniform)
                const int first = __ffsll((long long)live) - 1;
                const unsigned bref = (unsigned)__builtin_amdgcn_readlane((int)bl, first);
                if (__ballot(o != 0 && bl != bref) == 0) {
                    // one block: the largest ordered snr, then the smallest loc among the lanes that hold it (as k_ps_tiled, k_ffa_pass)
                    const unsigned mo = peakkey::wave_max(o);
                    const unsigned ml = peakkey::wave_min(o == mo ? loc : 0xFFFFFFFFu);
                    if (lane == first) atomicMax(&lkeys[bref], peakkey::key(mo, ml));
                } else if (o != 0) atomicMax(&lkeys[bl], peakkey::key(o, loc));
            }
        }
        __syncthreads();
        if (tid < nbl) {
            const u64 key = lkeys[tid];
            if (key) atomicMax(&keys[((size_t)s << (a.log2_nb - a.log2_bb)) + (size_t)(k0 >> a.log2_bb) + (size_t)tid], key);
        }
        __syncthreads();  // lkeys is free for the next unit
    }
}

// generic route: one thread per bin
__global__ __launch_bounds__(256) void k_ss_gen(const float *__restrict__ in, u64 *keys, long long total, int H, int log2_nb, int log2_bb,
                                                long long in_pitch)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long s = i >> log2_nb;
        const unsigned k = (unsigned)(i & ((1ll << log2_nb) - 1));
        const float *x = in + (size_t)s * (size_t)in_pitch;
        float acc = x[k];
        unsigned bo = 0, bh = 0;
        ss_fold(acc, 0, bo, bh);
        for (int h = 1; h <= H; h++) {
            for (unsigned j = 1; j < (1u << h); j += 2) acc = acc + x[ss_r(k, j, h)];
            ss_fold(acc, h, bo, bh);
        }
        if (bo != 0) {
            const unsigned loc = (bh << 24) | (k & ((1u << log2_bb) - 1));
            atomicMax(&keys[((size_t)s << (log2_nb - log2_bb)) + (size_t)(k >> log2_bb)], peakkey::key(bo, loc));
        }
    }
}

// record i of the [series][2^log2_nblk blocks] peaks buffer
struct SsSplit {
    __device__ __forceinline__ uint2 operator()(long long i, int log2_nblk) const
    {
        return make_uint2((unsigned)(i >> log2_nblk), (unsigned)(i & ((1ll << log2_nblk) - 1)));
    }
};

struct SsShape {
    int S, N, H, Bb, k_lo, kind;
};

int ss_log2(long long v)
{
    int l = 0;
    while ((1ll << l) < v) l++;
    return l;
}

bool ss_pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

// everything that can be told without a device
int ss_check(const SsShape &f)
{
    MI355_REQUIRE(f.S >= 1 && f.S <= kSsMaxS, "num_series must be 1 .. 2^20");
    MI355_REQUIRE(ss_pow2(f.N) && f.N >= (1 << kSsMinLog2N) && f.N <= (1 << kSsMaxLog2N), "n must be a power of two, 2^8 .. 2^22");
    MI355_REQUIRE(f.H >= 0 && f.H <= kSsMaxH, "num_folds must be 0 .. 5");
    MI355_REQUIRE(ss_pow2(f.Bb) && f.Bb >= kSsMinBb && f.Bb <= f.N / 2, "block_bins must be a power of two, 16 .. n / 2");
    MI355_REQUIRE(f.k_lo >= 1 && f.k_lo <= f.N / 2 - 1, "k_lo must be 1 .. n / 2 - 1");
    MI355_REQUIRE(f.kind == MI355_SSEARCH_SERIES || f.kind == MI355_SSEARCH_SPECTRUM, "input_kind must be SERIES (0) or SPECTRUM (1)");
    const long long row = f.kind == MI355_SSEARCH_SERIES ? f.N : f.N / 2;
    if ((long long)f.S * row > kSsMaxBytes / 4) {
        mi355_set_error("clSpectralSearch: %d series of %lld floats (the limit is 2^40 bytes per buffer)", f.S, row);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

// series per chunk of the spectrum stage
long long ss_chunk(const SsShape &f)
{
    const long long c = kSsChunkFloats / f.N;
    return c < 1 ? 1 : c > f.S ? f.S : c;
}

// SERIES input: per series of a chunk N floats of packed input, Nb complex bins and Nb floats of w
long long ss_scratch_bytes(const SsShape &f) { return f.kind == MI355_SSEARCH_SERIES ? ss_chunk(f) * 10ll * f.N : 0; }

}  // namespace

struct mi355_ssearch {
    mi355_ctx *ctx = nullptr;
    SsShape f = {};
    int Nb = 0, log2_nb = 0, log2_bb = 0, log2_tk = 0;
    long long nblk = 0, chunk = 1;
    bool generic = false;
    float threshold = INFINITY;
    std::vector<float> stats;  // inv_sigma S
    mi355_tables stab, twtab;  // the statistics (versioned) and the untangling twiddles (one version)
    mi355_fft *fft = nullptr;  // Nb points, complex, forward
    DevWorkspace ws;           // SERIES input: [packed x | Z | w] of a chunk, allocated by _create
    DevBuf d_in, d_out;        // host path
    std::string route;
    std::mutex lock;
};

namespace {

void ss_name_route(mi355_ssearch *h)
{
    char buf[320];
    int at = snprintf(buf, sizeof buf, "%s S=%d N=%d H=%d Bb=%d", h->generic ? "generic" : "tiled", h->f.S, h->f.N, h->f.H, h->f.Bb);
    if (!h->generic) at += snprintf(buf + at, sizeof buf - (size_t)at, " tk=%d", 1 << h->log2_tk);
    if (h->f.kind == MI355_SSEARCH_SERIES)
        snprintf(buf + at, sizeof buf - (size_t)at, " series k_lo=%d chunk=%lld fft=%d (packs through scratch when in_pitch != N, or fft > 4096 and `in` is not 16-byte aligned)", h->f.k_lo, h->chunk, h->Nb);
    else snprintf(buf + at, sizeof buf - (size_t)at, " spectrum");
    h->route = buf;
}

// the harmonic sums of nS series: w rows at w_pitch, keys at the first of them
void ss_sum(mi355_ssearch *h, const float *w, long long w_pitch, long long nS, u64 *keys, hipStream_t st)
{
    if (!h->generic) {
        SsArgs a = {};
        a.H = h->f.H; a.log2_nb = h->log2_nb; a.log2_bb = h->log2_bb; a.log2_tk = h->log2_tk; a.in_pitch = w_pitch;
        a.units = nS << (h->log2_nb - h->log2_tk);
        const long long cap = (long long)mi355_cus(h->ctx) * 4 * 4;  // four rounds of the resident workgroups
        hipLaunchKernelGGL(k_ss_tiled, dim3((unsigned)(a.units < cap ? a.units : cap)), dim3(kSsThreads), 0, st, w, keys, a);
    } else {
        const long long total = nS << h->log2_nb;
        hipLaunchKernelGGL(k_ss_gen, dim3(mi355_grid_256(h->ctx, total, 32)), dim3(256), 0, st, w, keys, total, h->f.H, h->log2_nb, h->log2_bb, w_pitch);
    }
}

// caller holds the lock and has set the device; series s0 .. s0 + nS - 1 of the handle, `in`, `peaks` and `spectrum` at the first of
// them; `series` of the candidate records counts from the launch's first series
int ss_launch(mi355_ssearch *h, long long s0, long long nS, const void *in, long long in_pitch, void *peaks, float *spectrum, void *cands,
              long long max_cands, void *counts, hipStream_t st)
{
    const SsShape &f = h->f;
    const long long nrec = nS * h->nblk;
    u64 *keys = (u64 *)peaks;
    hipLaunchKernelGGL(peakkey::k_peak_init<>, dim3(mi355_grid_256(h->ctx, nrec, 32)), dim3(256), 0, st, keys, nrec, cands ? (unsigned *)counts : nullptr);
    if (f.kind == MI355_SSEARCH_SPECTRUM) ss_sum(h, (const float *)in, in_pitch, nS, keys, st);
    else {
        int rc = h->ws.acquire(h->ws.bytes(), st);  // the size of _create: nothing is allocated here
        if (rc) return rc;
        const long long N = f.N, Nb = h->Nb;
        float *d_pack = (float *)h->ws.get();
        float2 *d_z = (float2 *)(d_pack + h->chunk * N);
        float *d_w = (float *)(d_z + h->chunk * Nb);
        const float *d_isg = (const float *)h->stab.current() + s0;
        // clFFT takes a device input of more than 4096 points at a 16-byte boundary only
        const bool pack = in_pitch != N || (Nb > 4096 && (reinterpret_cast<uintptr_t>(in) & 15u) != 0);
        for (long long c0 = 0; c0 < nS; c0 += h->chunk) {
            const long long nc = nS - c0 < h->chunk ? nS - c0 : h->chunk;
            const float *src = (const float *)in + c0 * in_pitch;
            if (pack) {
                hipLaunchKernelGGL(k_ss_pack, dim3(mi355_grid_256(h->ctx, nc * Nb, 32)), dim3(256), 0, st, (const float2 *)src, in_pitch / 2,
                                   (float2 *)d_pack, nc * Nb, h->log2_nb);
                src = d_pack;
            }
            if ((rc = mi355_fft_work_dev(h->fft, (int)nc, src, d_z, (void *)st))) return rc;
            float *w = spectrum ? spectrum + c0 * Nb : d_w;
            hipLaunchKernelGGL(k_ss_power, dim3(mi355_grid_256(h->ctx, nc * (Nb / 2), 32)), dim3(256), 0, st, (const float2 *)d_z,
                               (const float2 *)h->twtab.current(), d_isg + c0, w, nc * (Nb / 2), h->log2_nb, f.k_lo, 1.0f / (float)N);
            ss_sum(h, w, Nb, nc, keys + c0 * h->nblk, st);
        }
        if ((rc = h->ws.release(st))) return rc;
    }
    hipLaunchKernelGGL(peakkey::k_peak_emit<SsSplit>, dim3(mi355_grid_256(h->ctx, nrec, 32)), dim3(256), 0, st, keys, nrec, ss_log2(h->nblk), h->threshold, (uint2 *)cands,
                       max_cands, (unsigned *)counts);
    MI355_HIP(hipGetLastError());
    if (f.kind == MI355_SSEARCH_SERIES) return h->stab.used(st);  // this version of the statistics may be released behind these launches
    return MI355_OK;
}

int ss_args(const mi355_ssearch *h, const void *in, long long in_pitch, const void *peaks, const void *spectrum, const void *cands,
            long long max_cands, const void *counts)
{
    const bool series = h->f.kind == MI355_SSEARCH_SERIES;
    const long long S = h->f.S, row = series ? h->f.N : h->Nb;
    MI355_REQUIRE(in && peaks, "NULL buffer");
    MI355_REQUIRE(max_cands >= 0, "max_cands is negative");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & (series ? 7u : 3u)) == 0, "in must be 8-byte (SERIES) or 4-byte (SPECTRUM) aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(peaks) & 7u) == 0, "peaks must be 8-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(spectrum) & 3u) == 0, "spectrum must be 4-byte aligned");
    MI355_REQUIRE(series || !spectrum, "a spectrum output with SPECTRUM input");
    if (const int rc = peakkey::check_cands(cands, counts)) return rc;
    MI355_REQUIRE(in_pitch >= row, "in_pitch is below the floats of a series");
    MI355_REQUIRE(!series || (in_pitch & 1) == 0, "in_pitch must be even with SERIES input");
    if (in_pitch > kSsMaxBytes / (4 * S) || max_cands > kSsMaxBytes / 16) {
        mi355_set_error("clSpectralSearch: %lld series of pitch %lld, %lld candidates (the limit is 2^40 bytes per buffer)", S, in_pitch, max_cands);
        return MI355_ERR_UNSUPPORTED;
    }
    const long long ib = 4 * ((S - 1) * in_pitch + row), pb = 8 * S * h->nblk, sb = 4 * S * h->Nb, cb = 16 * max_cands;
    MI355_REQUIRE(!mi355_overlap(in, ib, peaks, pb), "clSpectralSearch does not work in place: in and peaks overlap");
    if (spectrum) {
        MI355_REQUIRE(!mi355_overlap(in, ib, spectrum, sb), "in and spectrum overlap");
        MI355_REQUIRE(!mi355_overlap(peaks, pb, spectrum, sb), "peaks and spectrum overlap");
    }
    if (const int rc = peakkey::check_cands_apart(in, ib, peaks, pb, cands, max_cands, counts)) return rc;
    if (cands && spectrum) {
        MI355_REQUIRE(max_cands == 0 || !mi355_overlap(spectrum, sb, cands, cb), "spectrum and cands overlap");
        MI355_REQUIRE(!mi355_overlap(spectrum, sb, counts, 8), "spectrum and counts overlap");
    }
    return MI355_OK;
}

// (cos, sin)(2 pi k / N) for k = 0 .. N / 4, each from an argument of at most pi / 4 in double: exact 0 and 1 at the ends, the same
// value where the octants meet, within half a binary32 unit (and the error of the double) everywhere
void ss_twiddles(int N, std::vector<float> *tw)
{
    const int q = N / 4;
    tw->resize(2 * (size_t)(q + 1));
    for (int k = 0; k <= q; k++) {
        double c, s;
        if (2 * k <= q) {
            const double a = 2.0 * M_PI * (double)k / (double)N;
            c = cos(a); s = sin(a);
        } else {
            const double a = 2.0 * M_PI * (double)(q - k) / (double)N;
            c = sin(a); s = cos(a);
        }
        (*tw)[2 * (size_t)k] = (float)c;
        (*tw)[2 * (size_t)k + 1] = (float)s;
    }
}

}  // namespace

extern "C" int mi355_ssearch_plan(int num_series, int n, int num_folds, int block_bins, int k_lo, int input_kind, long long *spectrum_floats_per_series,
                                  long long *records_per_series, long long *scratch_bytes)
{
    if (spectrum_floats_per_series) *spectrum_floats_per_series = 0;
    if (records_per_series) *records_per_series = 0;
    if (scratch_bytes) *scratch_bytes = 0;
    const SsShape f = {num_series, n, num_folds, block_bins, k_lo, input_kind};
    const int rc = ss_check(f);
    if (rc) return rc;
    if (spectrum_floats_per_series) *spectrum_floats_per_series = f.N / 2;
    if (records_per_series) *records_per_series = f.N / 2 / f.Bb;
    if (scratch_bytes) *scratch_bytes = ss_scratch_bytes(f);
    return MI355_OK;
}

extern "C" int mi355_ssearch_create(mi355_ctx *ctx, int num_series, int n, int num_folds, int block_bins, int k_lo, int input_kind,
                                    const float *inv_sigma, mi355_ssearch **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    const SsShape f = {num_series, n, num_folds, block_bins, k_lo, input_kind};
    int rc = ss_check(f);
    if (rc) return rc;
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_ssearch *h = new (std::nothrow) mi355_ssearch();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->f = f; h->Nb = f.N / 2; h->log2_nb = ss_log2(h->Nb); h->log2_bb = ss_log2(f.Bb);
    h->log2_tk = h->Nb < kSsMaxTk ? h->log2_nb : ss_log2(kSsMaxTk);
    h->nblk = h->Nb / f.Bb;
    h->chunk = ss_chunk(f);
    const size_t S = (size_t)f.S;
    h->stats.assign(S, 1.0f);
    if (inv_sigma) memcpy(h->stats.data(), inv_sigma, S * 4);
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_ssearch_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else if (f.kind == MI355_SSEARCH_SERIES) {
        std::vector<float> tw;
        ss_twiddles(f.N, &tw);
        rc = h->stab.publish(ctx, h->stats.data(), S * 4, "mi355_ssearch: statistics");
        if (rc == MI355_OK) rc = h->twtab.publish(ctx, tw.data(), tw.size() * 4, "mi355_ssearch: twiddles");
        if (rc == MI355_OK) rc = mi355_fft_create(ctx, h->Nb, MI355_FFT_FORWARD, nullptr, 0, MI355_DTYPE_COMPLEX, 1, 0, &h->fft);
        if (rc == MI355_OK) rc = h->ws.acquire((size_t)ss_scratch_bytes(f), ctx->stream[0]);
        if (rc == MI355_OK) {
            // one transform of a whole chunk of zeros: whatever workspace the internal handle needs for a chunk is allocated now
            const size_t zb = (size_t)(h->chunk * f.N * 4);
            hipError_t fe = mi355_fill(ctx, h->ws.get(), 0, zb);
            if (fe == hipSuccess) {
                rc = mi355_fft_work_dev(h->fft, (int)h->chunk, h->ws.get(), (char *)h->ws.get() + zb, (void *)ctx->stream[0]);
                if (rc == MI355_OK) rc = h->ws.release(ctx->stream[0]);
                fe = hipStreamSynchronize(ctx->stream[0]);
            }
            if (fe != hipSuccess) {
                mi355_set_error("mi355_ssearch_create: %s", hipGetErrorString(fe));
                rc = MI355_ERR_HIP;
            }
        }
    }
    if (rc) { mi355_ssearch_destroy(h); return rc; }
    ss_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clSpectralSearch: %d series of %d samples, %d folds, blocks of %d bins: %s", f.S, f.N, f.H, f.Bb, h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_ssearch_destroy(mi355_ssearch *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)h->ws.wait();
    if (h->fft) (void)mi355_fft_destroy(h->fft);
    h->ws.destroy();
    h->stab.release();
    h->twtab.release();
    h->d_in.release();
    h->d_out.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_ssearch_set_stats(mi355_ssearch *h, const float *inv_sigma)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(inv_sigma != nullptr, "inv_sigma is NULL");
    const size_t S = (size_t)h->f.S;
    std::vector<float> img(inv_sigma, inv_sigma + S);
    std::lock_guard<std::mutex> g(h->lock);
    if (h->f.kind == MI355_SSEARCH_SERIES) {
        MI355_HIP(hipSetDevice(h->ctx->device));
        const int rc = h->stab.publish(h->ctx, img.data(), S * 4, "mi355_ssearch: statistics");  // on failure the version in use stays
        if (rc) return rc;
    }
    h->stats.swap(img);
    return MI355_OK;
}

extern "C" int mi355_ssearch_get_stats(const mi355_ssearch *h, float *inv_sigma, long long cap_entries)
{
    MI355_REQUIRE(h && inv_sigma, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_ssearch *>(h)->lock);
    MI355_REQUIRE(cap_entries >= (long long)h->f.S, "out too small");
    memcpy(inv_sigma, h->stats.data(), (size_t)h->f.S * 4);
    return MI355_OK;
}

extern "C" int mi355_ssearch_set_threshold(mi355_ssearch *h, float threshold)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(threshold == threshold, "threshold is NaN");
    std::lock_guard<std::mutex> g(h->lock);
    h->threshold = threshold;
    return MI355_OK;
}

extern "C" int mi355_ssearch_set_generic(mi355_ssearch *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    ss_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_ssearch_route(const mi355_ssearch *h) { return h ? h->route.c_str() : ""; }

extern "C" const char *mi355_ssearch_fft_route(const mi355_ssearch *h) { return h && h->fft ? mi355_fft_last_route(h->fft) : ""; }

extern "C" int mi355_ssearch_work_dev(mi355_ssearch *h, const void *in, long long in_pitch, void *peaks, void *spectrum, void *cands,
                                      long long max_cands, void *counts, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = ss_args(h, in, in_pitch, peaks, spectrum, cands, max_cands, counts);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return ss_launch(h, 0, h->f.S, in, in_pitch, peaks, (float *)spectrum, cands, max_cands, counts, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_ssearch_work(mi355_ssearch *h, const void *in, long long in_pitch, void *peaks, void *spectrum, void *cands, long long max_cands,
                                  void *counts)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = ss_args(h, in, in_pitch, peaks, spectrum, cands, max_cands, counts);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole series; the records, the counter, the candidates and the spectra of a piece lie behind one another in d_out.
    // The candidates of a piece come back in a list of their own and are appended with `series` counted from the call's first
    const long long S = h->f.S, row = h->f.kind == MI355_SSEARCH_SERIES ? h->f.N : h->Nb;
    const long long piece = mi355_piece_units(kSsHostBytes / (4 * row), S);
    const long long peak_bytes = 8 * h->nblk, spec_bytes = spectrum ? 4ll * h->Nb : 0, cand_bytes = cands ? 16 * max_cands : 0;
    if ((rc = h->d_in.reserve((size_t)(4 * row * piece)))) return rc;
    if ((rc = h->d_out.reserve((size_t)(piece * peak_bytes + 8 + cand_bytes + piece * spec_bytes)))) return rc;
    char *d_peaks = (char *)h->d_out.get(), *d_counts = d_peaks + piece * peak_bytes, *d_cands = d_counts + 8, *d_spec = d_cands + cand_bytes;
    peakkey::CandList list(cands, max_cands);
    rc = mi355_pageable_run(h->ctx, S, piece, [&](long long s0, long long ns, hipStream_t st) -> int {
        MI355_HIP(hipMemcpy2DAsync(h->d_in.get(), (size_t)(4 * row), (const float *)in + s0 * in_pitch, (size_t)(4 * in_pitch), (size_t)(4 * row), (size_t)ns,
                                   hipMemcpyHostToDevice, st));
        const int lrc = ss_launch(h, s0, ns, h->d_in.get(), row, d_peaks, spectrum ? (float *)d_spec : nullptr, cands ? d_cands : nullptr, max_cands,
                                  d_counts, st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)peaks + s0 * peak_bytes, d_peaks, (size_t)(ns * peak_bytes), hipMemcpyDeviceToHost, st));
        if (spectrum) MI355_HIP(hipMemcpyAsync((char *)spectrum + s0 * spec_bytes, d_spec, (size_t)(ns * spec_bytes), hipMemcpyDeviceToHost, st));
        return cands ? list.append(d_counts, d_cands, peakkey::CandList::SERIES, s0, st) : MI355_OK;
    });
    if (rc) return rc;
    if (cands) list.finish(counts);
    return MI355_OK;
}

// host only: the fundamental of harmonic-sum level h at bin k, k / (2^h N tsamp) in Hz; NaN for arguments outside the ranges
extern "C" double mi355_ssearch_freq(int n, double tsamp_s, int h, int k)
{
    if (!ss_pow2(n) || n < (1 << kSsMinLog2N) || n > (1 << kSsMaxLog2N) || h < 0 || h > kSsMaxH || k < 0 || k >= n / 2 || !(tsamp_s > 0.0) ||
        !std::isfinite(tsamp_s))
        return NAN;
    return (double)k / ((double)(1 << h) * (double)n * tsamp_s);
}
