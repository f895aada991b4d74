// clPeriodSearch: exact fast-folding search (FFA, Staelin 1969) for unknown periods over the S dedispersed time series that clDedisperser
// delivers, as gfx950 HIP kernels.  The contract is in include/mi355_clenabled.h; the reference module has no such block.
//
//     a_0[r] = row r of p bins;   a_s[B + i][j] = a_(s-1)[B + (i>>1)][j] + a_(s-1)[B + h + (i>>1)][(j + ((i+1)>>1)) mod p]   (g = 2^s, h = g/2)
//     b_0 = a_L[i],  b_k[j] = b_(k-1)[j] + b_(k-1)[(j + 2^(k-1)) mod p];   snr_k[j] = (b_k[j] - mean 2^(L+k)) (inv_sigma c_(L+k))
//     record of trial (s, p, i) = the largest 64-bit key {order-preserving map of snr's bits, ~((k << 24) | j)} over k and j
//
// Every value is one binary32 addition of two fixed operands, so the partition of the stages into passes changes nothing.
//
// k_ffa_pass   the fused route.  Stages a+1 .. a+q of a group of 2^(a+q) rows fall apart into 2^a independent units: the 2^q output rows
//              with u = i >> q depend on row u of each of the 2^q sub-groups of 2^a rows.  A workgroup owns one unit: it gathers the 2^q
//              rows into LDS (row pitch p: lanes run along j, the axis of the circular shift, so a group of 32 lanes reads 32 consecutive
//              dwords of a row except where the shift wraps), and runs the q stages there.  A thread owns pairs (output rows 2v, 2v+1,
//              bin j): it reads the head once and the tail at two neighbouring shifts, keeps both sums in registers, all threads meet
//              at a barrier, then the sums replace the stage's input -- both operands of every sum come from the previous stage.  The
//              unit's rows are contiguous in the destination plane.  The last pass writes the profiles (if asked), builds the boxcar
//              levels in place in the same way (own value in a register, partner from LDS, barrier, store), folds snr_k into each
//              bin's running (ordered snr, k), reduces a wave's keys with DPP row operations when its lanes lie in one row and with
//              64-bit LDS atomicMax otherwise and across waves, and writes one record per row.  No global atomics, no init, no emit.
// k_ffa_stage  the generic route: one launch per stage, one thread per output, between two scratch planes.
// k_ffa_eval   the generic route's evaluation: one wave per trial; a lane walks the tree of the widest boxcar of its bins leaf by leaf.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"
#include "peakkey.hpp"

#pragma clang fp contract(off)

namespace {

using peakkey::u64;

constexpr int kFfaMaxS = 1 << 20, kFfaMinP = 16, kFfaMaxP = 4096, kFfaMaxL = 12, kFfaMaxK = 11;
constexpr long long kFfaMaxBytes = 1ll << 40;
constexpr long long kFfaHostBytes = 4ll << 20;    // host path: input bytes per staged piece unless one series needs more
constexpr long long kFfaBatchFloats = 1ll << 23;  // base periods share a launch while a scratch plane stays below this (32 MiB)
constexpr int kFfaPairs = 16;                     // (head, tail) pairs a thread of k_ffa_pass owns: 32 sums in registers
constexpr int kFfaEval = 8;                       // bins a thread owns per evaluation chunk; a chunk holds whole rows, so threads x 8 >= p
constexpr int kFfaSmallPairs = 256 * kFfaPairs, kFfaLargePairs = 1024 * kFfaPairs;  // pairs of a unit: 256 or 1024 threads
constexpr int kFfaMaxQ = 8;

// snr of one sum at level e = L + k folded into the running best of its bin under the tag k (peakkey.hpp has the key)
__device__ __forceinline__ void ffa_fold(float b, int e, int k, float mean, float isg, unsigned &bo, unsigned &bk)
{
    const float m = mean * (float)(1 << e);
    const float g = isg * peakkey::c(e);
    const float d = b - m;
    peakkey::fold(d * g, k, bo, bk);
}

// e = l p + j with j < p, for magic = floor(2^32 / p): mulhi gives l or one less
__device__ __forceinline__ void ffa_div(unsigned e, unsigned p, unsigned magic, unsigned &l, unsigned &j)
{
    l = __umulhi(e, magic);
    j = e - l * p;
    if (j >= p) { l++; j -= p; }
}

struct FfaArgs {
    int S, Sst;             // series of this launch; distance from mean[s] to inv_sigma[s] in stats
    int L, K, m, p_lo, p_hi, P;
    int p0, np;             // base periods p0 .. p0 + np - 1 in this launch
    int a, q;               // stages a+1 .. a+q
    int first, last;
    long long in_pitch;
    long long slot;         // floats per (period of the launch, series) in a scratch plane: m p_hi; its rows have pitch p
    long long units;
};

// in: the call's input (first pass);  src / dst: scratch planes;  peaks / profiles: the call's outputs at series 0 of this launch
template <int THREADS>
__global__ __launch_bounds__(THREADS, 4) void k_ffa_pass(const float *__restrict__ in, const float *__restrict__ src, float *__restrict__ dst,
                                                      const float *__restrict__ stats, uint2 *__restrict__ peaks, float *__restrict__ profiles,
                                                      const FfaArgs a)
{
    // [rows] keys, [rows] shifts of the stage, then rows x p floats
    extern __shared__ __attribute__((aligned(16))) u64 lkeys[];
    const int rows = 1 << a.q;
    int *shl = (int *)(lkeys + rows);
    float *lds = (float *)(shl + rows);
    const int tid = threadIdx.x, lane = tid & 63;
    const int per = a.m >> a.q;  // units per (period, series)
    for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const int w = (int)(unit % per);
        const long long ps = unit / per;
        const int s = (int)(ps % a.S), pi = (int)(ps / a.S);
        const int u = w & ((1 << a.a) - 1), B = (w >> a.a) << (a.a + a.q);
        const unsigned p = (unsigned)(a.p0 + pi), tot = (unsigned)rows * p, half = tot >> 1;
        const unsigned magic = (unsigned)((1ull << 32) / p);
        const size_t slot = ((size_t)pi * (size_t)a.S + (size_t)s) * (size_t)a.slot;
        if (tid < rows) lkeys[tid] = 0;
        if (tid < rows / 2) shl[tid] = (int)((unsigned)u % p);  // stage 1 of the pass: h = 1, v = 0, shift (u h + v) mod p
        if (a.first) {
            const float *x = in + (size_t)s * (size_t)a.in_pitch + (size_t)B * p;  // u = 0: the unit's rows are contiguous
#pragma unroll 4
            for (unsigned e = tid; e < tot; e += THREADS) lds[e] = x[e];
        } else {
            const float *x = src + slot + (size_t)(B + u) * p;
            const size_t rstride = (size_t)p << a.a;
#pragma unroll 4
            for (unsigned e = tid; e < tot; e += THREADS) {
                unsigned l, j;
                ffa_div(e, p, magic, l, j);
                lds[e] = x[(size_t)l * rstride + j];
            }
        }
        unsigned pj[kFfaPairs];  // (pair << 16) | j
#pragma unroll
        for (int n = 0; n < kFfaPairs; n++) {
            unsigned l, j;
            ffa_div((unsigned)(tid + THREADS * n), p, magic, l, j);
            pj[n] = (l << 16) | j;
        }
        __syncthreads();
        for (int t = 1; t <= a.q; t++) {
            const unsigned h = 1u << (t - 1);
            float r0[kFfaPairs], r1[kFfaPairs];
#pragma unroll
            for (int n = 0; n < kFfaPairs; n++) {
                if ((unsigned)(tid + THREADS * n) < half) {
                    const unsigned pr = pj[n] >> 16, j = pj[n] & 0xFFFFu, v = pr & (h - 1), hd = 2 * pr - v;
                    unsigned x = j + (unsigned)shl[pr];
                    x -= x >= p ? p : 0u;
                    unsigned y = x + 1;
                    y = y == p ? 0u : y;
                    const unsigned at = __umul24(hd, p);  // (every product here is below 2^16: full-rate 24-bit multiplies)
                    const float *tail = lds + at + __umul24(h, p);
                    const float H = lds[at + j];
                    r0[n] = H + tail[x];
                    r1[n] = H + tail[y];
                }
            }
            __syncthreads();  // every operand of the stage has been read
#pragma unroll
            for (int n = 0; n < kFfaPairs; n++) {
                if ((unsigned)(tid + THREADS * n) < half) {
                    const unsigned pr = pj[n] >> 16, j = pj[n] & 0xFFFFu, o = __umul24(2 * pr, p) + j;  // rows 2 pr and 2 pr + 1
                    lds[o] = r0[n];
                    lds[o + p] = r1[n];
                }
            }
            if (tid < rows / 2) shl[tid] = (int)((((unsigned)u << t) + ((unsigned)tid & (2 * h - 1))) % p);  // stage t + 1
            __syncthreads();
        }
        if (!a.last) {
            float *y = dst + slot + ((size_t)B + ((size_t)u << a.q)) * p;
            for (unsigned e = tid; e < tot; e += THREADS) y[e] = lds[e];
        } else {
            const int i0 = u << a.q;  // the group is the whole series: B = 0
            const size_t trial0 = ((size_t)s * (size_t)a.P + (size_t)(a.p0 - a.p_lo + pi)) * (size_t)a.m + (size_t)i0;
            if (profiles) {
                float *y = profiles + trial0 * (size_t)a.p_hi;
                for (unsigned e = tid; e < tot; e += THREADS) {
                    unsigned l, j;
                    ffa_div(e, p, magic, l, j);
                    y[(size_t)l * (size_t)a.p_hi + j] = lds[e];
                }
            }
            const float mean = stats[s], isg = stats[a.Sst + s];
            const unsigned rpc = (unsigned)(THREADS * kFfaEval) / p;  // rows per chunk, >= 1
            for (unsigned row0 = 0; row0 < (unsigned)rows; row0 += rpc) {
                const unsigned nr = (unsigned)rows - row0 < rpc ? (unsigned)rows - row0 : rpc, cnt = nr * p, base = row0 * p;
                float r[kFfaEval];
                unsigned bo[kFfaEval], kj[kFfaEval], lj[kFfaEval];  // best ordered snr; its k; (row in chunk << 16) | j
#pragma unroll
                for (int n = 0; n < kFfaEval; n++) {
                    const unsigned e = (unsigned)(tid + THREADS * n);
                    unsigned l, j;
                    ffa_div(e, p, magic, l, j);
                    lj[n] = (l << 16) | j;
                    r[n] = e < cnt ? lds[base + e] : 0.0f;
                    bo[n] = 0;
                    kj[n] = 0;
                    ffa_fold(r[n], a.L, 0, mean, isg, bo[n], kj[n]);
                }
                for (int k = 1; k < a.K; k++) {
                    const unsigned h = 1u << (k - 1);
                    float q[kFfaEval];
#pragma unroll
                    for (int n = 0; n < kFfaEval; n++) {
                        const unsigned e = (unsigned)(tid + THREADS * n), j = lj[n] & 0xFFFFu;
                        q[n] = e < cnt ? lds[base + e + h - (j + h >= p ? p : 0u)] : 0.0f;
                    }
                    __syncthreads();  // every partner has been read
#pragma unroll
                    for (int n = 0; n < kFfaEval; n++) {
                        const unsigned e = (unsigned)(tid + THREADS * n);
                        r[n] = r[n] + q[n];
                        ffa_fold(r[n], a.L + k, k, mean, isg, bo[n], kj[n]);
                        if (e < cnt) lds[base + e] = r[n];
                    }
                    __syncthreads();  // level k is in place
                }
#pragma unroll
                for (int n = 0; n < kFfaEval; n++) {
                    const unsigned e = (unsigned)(tid + THREADS * n);
                    const unsigned o = e < cnt ? bo[n] : 0u;  // 0: nothing to report
                    const unsigned row = row0 + (lj[n] >> 16), loc = (kj[n] << 24) | (lj[n] & 0xFFFFu);
                    const u64 live = __ballot(o != 0);
                    if (live) {  // (uniform)
                        const int firstl = __ffsll((long long)live) - 1;
                        const unsigned rref = (unsigned)__builtin_amdgcn_readlane((int)row, firstl);
                        if (__ballot(o != 0 && row != rref) == 0) {
                            // one row: the largest ordered snr, then the smallest loc among the lanes that hold it (as k_ps_tiled, k_ss_tiled)
                            const unsigned mo = peakkey::wave_max(o);
                            const unsigned ml = peakkey::wave_min(o == mo ? loc : 0xFFFFFFFFu);
                            if (lane == firstl) atomicMax(&lkeys[rref], peakkey::key(mo, ml));
                        } else if (o != 0) atomicMax(&lkeys[row], peakkey::key(o, loc));
                    }
                }
            }
            __syncthreads();
            if (tid < rows) peaks[trial0 + (size_t)tid] = peakkey::record(lkeys[tid]);
        }
        __syncthreads();  // the rows, the shifts and the keys are free for the next unit
    }
}

// generic route, stage sg: src rows of pitch p, series pitch src_pitch (the input for sg = 1, a scratch plane after that)
__global__ __launch_bounds__(256) void k_ffa_stage(const float *__restrict__ src, long long src_pitch, float *__restrict__ dst, long long dst_pitch, int S,
                                                   int m, int p, int sg)
{
    const long long mp = (long long)m * p, total = (long long)S * mp;
    const int g = 1 << sg, h = g >> 1;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long s = idx / mp;
        const int e = (int)(idx - s * mp), row = e / p, j = e - row * p;
        const int i = row & (g - 1), B = row - i;
        int jj = j + ((i + 1) >> 1) % p;
        jj -= jj >= p ? p : 0;
        const float *x = src + (size_t)s * (size_t)src_pitch;
        dst[(size_t)s * (size_t)dst_pitch + (size_t)row * p + j] = x[(size_t)(B + (i >> 1)) * p + j] + x[(size_t)(B + h + (i >> 1)) * p + jj];
    }
}

// generic route, evaluation of base period p: one wave per trial (s, i); y: the last stage's plane
__global__ __launch_bounds__(256) void k_ffa_eval(const float *__restrict__ y, long long y_pitch, const float *__restrict__ stats, int Sst,
                                                  uint2 *__restrict__ peaks, float *__restrict__ profiles, int S, int L, int K, int p, int pidx, int P,
                                                  int p_hi)
{
    const int m = 1 << L, lane = threadIdx.x & 63;
    const long long trials = (long long)S * m, waves = (long long)gridDim.x * 4;
    const int width = 1 << (K - 1);
    for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < trials; t += waves) {
        const long long s = t / m;
        const int i = (int)(t - s * m);
        const float *row = y + (size_t)s * (size_t)y_pitch + (size_t)i * p;
        const size_t trial = ((size_t)s * (size_t)P + (size_t)pidx) * (size_t)m + (size_t)i;
        const float mean = stats[s], isg = stats[Sst + s];
        u64 key = 0;
        for (int j = lane; j < p; j += 64) {
            if (profiles) profiles[trial * (size_t)p_hi + j] = row[j];
            unsigned bo = 0, bk = 0;
            float st[kFfaMaxK];
#pragma unroll
            for (int l = 0; l < kFfaMaxK; l++) st[l] = 0.0f;
            // leaf f of the tree over row[(j + f) mod p], f < 2^(K-1): merge while the counter carries.  The node finished at leaf
            // 2^l - 1 is b_l[j]
            for (int f = 0; f < width; f++) {
                int at = j + f;
                at -= at >= p ? p : 0;
                float v = row[at];
                bool open = true;
#pragma unroll
                for (int l = 0; l < kFfaMaxK; l++) {
                    if (open) {
                        if ((f >> l) & 1) v = st[l] + v;
                        else {
                            st[l] = v;
                            open = false;
                            if (f + 1 == (1 << l)) ffa_fold(v, L + l, l, mean, isg, bo, bk);
                        }
                    }
                }
            }
            const u64 mine = bo ? peakkey::key(bo, (bk << 24) | (unsigned)j) : 0;
            key = mine > key ? mine : key;
        }
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned hi = (unsigned)__shfl_xor((int)(key >> 32), d), lo = (unsigned)__shfl_xor((int)(unsigned)key, d);
            const u64 other = ((u64)hi << 32) | lo;
            key = other > key ? other : key;
        }
        if (lane == 0) peaks[trial] = peakkey::record(key);
    }
}

struct FfaShape {
    int S, p_lo, p_hi, L, K;
};

// everything that can be told without a device
int ffa_check(const FfaShape &f)
{
    MI355_REQUIRE(f.S >= 1 && f.S <= kFfaMaxS, "num_series must be 1 .. 2^20");
    MI355_REQUIRE(f.p_lo >= kFfaMinP && f.p_lo <= f.p_hi && f.p_hi <= kFfaMaxP, "base periods must satisfy 16 <= p_lo <= p_hi <= 4096");
    MI355_REQUIRE(f.L >= 1 && f.L <= kFfaMaxL, "log2_rows must be 1 .. 12");
    MI355_REQUIRE(f.K >= 1 && f.K <= kFfaMaxK, "num_widths must be 1 .. 11");
    MI355_REQUIRE((1 << (f.K - 1)) <= f.p_lo, "the widest boxcar 2^(num_widths-1) must not exceed p_lo");
    const long long m = 1ll << f.L, P = f.p_hi - f.p_lo + 1;
    if ((long long)f.S * m * f.p_hi > kFfaMaxBytes / 4 || (long long)f.S * P * m > kFfaMaxBytes / 8) {
        mi355_set_error("clPeriodSearch: %d series of %lld rows of up to %d bins, %lld base periods (the limit is 2^40 bytes per buffer)", f.S, m, f.p_hi, P);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

// base periods per launch of the fused route, and with it the floats of one scratch plane
long long ffa_batch(const FfaShape &f)
{
    const long long per = (long long)f.S * ((long long)f.p_hi << f.L), P = f.p_hi - f.p_lo + 1;
    const long long b = kFfaBatchFloats / per;
    return b < 1 ? 1 : b > P ? P : b;
}

long long ffa_scratch_bytes(const FfaShape &f) { return 2 * 4 * ffa_batch(f) * (long long)f.S * ((long long)f.p_hi << f.L); }

}  // namespace

struct mi355_ffa {
    mi355_ctx *ctx = nullptr;
    FfaShape f = {};
    int m = 0, P = 0;
    long long N = 0;
    int npass = 0, q[kFfaMaxL] = {};  // the fused route's passes
    int threads = 0, lds_bytes = 0;
    long long batch = 1;
    bool generic = false;
    peakkey::SeriesStats stats;
    DevWorkspace ws;           // two scratch planes, allocated by _create
    DevBuf d_in, d_out;        // host path
    std::string route;
    std::mutex lock;
};

namespace {

void ffa_plan(mi355_ffa *h)
{
    // the most stages per pass: 2^q rows of p_hi floats in LDS, a thread owns at most kFfaPairs pairs
    int qmax = 1;
    while (qmax < kFfaMaxQ && ((1ll << qmax) * h->f.p_hi) <= kFfaLargePairs) qmax++;
    const int L = h->f.L;
    h->npass = (L + qmax - 1) / qmax;
    for (int i = 0; i < h->npass; i++) h->q[i] = L / h->npass + (i < L % h->npass ? 1 : 0);  // as even as L allows, the larger ones first
    const int rows = 1 << h->q[0];
    h->threads = (rows / 2) * h->f.p_hi <= kFfaSmallPairs && h->f.p_hi <= 256 * kFfaEval ? 256 : 1024;
    h->lds_bytes = rows * 12 + rows * h->f.p_hi * 4;
    h->batch = ffa_batch(h->f);
}

void ffa_name_route(mi355_ffa *h)
{
    char buf[200];
    int at = snprintf(buf, sizeof buf, "%s S=%d p=%d..%d L=%d K=%d", h->generic ? "generic" : "fused", h->f.S, h->f.p_lo, h->f.p_hi, h->f.L, h->f.K);
    if (!h->generic) {
        for (int i = 0; i < h->npass; i++) at += snprintf(buf + at, sizeof buf - (size_t)at, "%s%d", i ? "," : " q=", h->q[i]);
        snprintf(buf + at, sizeof buf - (size_t)at, " t=%d", h->threads);
    }
    h->route = buf;
}

// caller holds the lock and has set the device; series s0 .. s0 + nS - 1 of the handle, `in`, `peaks` and `profiles` at the first of them
int ffa_launch(mi355_ffa *h, int s0, int nS, const float *in, long long in_pitch, uint2 *peaks, float *profiles, hipStream_t st)
{
    const FfaShape &f = h->f;
    const float *d_stats = h->stats.current() + s0;
    int rc = h->ws.acquire(h->ws.bytes(), st);  // the size of _create: nothing is allocated here
    if (rc) return rc;
    const long long slot = (long long)h->m * f.p_hi;
    float *plane[2] = {(float *)h->ws.get(), (float *)h->ws.get() + h->ws.bytes() / 8};
    if (!h->generic) {
        FfaArgs a = {};
        a.S = nS; a.Sst = f.S; a.L = f.L; a.K = f.K; a.m = h->m; a.p_lo = f.p_lo; a.p_hi = f.p_hi; a.P = h->P;
        a.in_pitch = in_pitch; a.slot = slot;
        const void *fn = h->threads == 256 ? (const void *)k_ffa_pass<256> : (const void *)k_ffa_pass<1024>;
        if (h->lds_bytes > (64 << 10)) MI355_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes));
        const int per_cu = h->threads == 256 ? (h->lds_bytes > (40 << 10) ? 2 : h->lds_bytes > (20 << 10) ? 4 : 8) : 1;
        const long long cap = (long long)mi355_cus(h->ctx) * per_cu * 4;  // four rounds of the resident workgroups
        for (int pb = 0; pb < h->P; pb += (int)h->batch) {
            a.p0 = f.p_lo + pb;
            a.np = h->P - pb < (int)h->batch ? h->P - pb : (int)h->batch;
            a.a = 0;
            for (int i = 0; i < h->npass; i++) {
                a.q = h->q[i];
                a.first = i == 0;
                a.last = i == h->npass - 1;
                a.units = (long long)a.np * nS * (h->m >> a.q);
                const dim3 grid((unsigned)(a.units < cap ? a.units : cap));
                const int lds = (1 << a.q) * 12 + (1 << a.q) * (a.p0 + a.np - 1) * 4;
                const float *src = plane[(i + 1) & 1];
                float *dst = plane[i & 1];
                if (h->threads == 256) hipLaunchKernelGGL(k_ffa_pass<256>, grid, dim3(256), (size_t)lds, st, in, src, dst, d_stats, peaks, profiles, a);
                else hipLaunchKernelGGL(k_ffa_pass<1024>, grid, dim3(1024), (size_t)lds, st, in, src, dst, d_stats, peaks, profiles, a);
                a.a += a.q;
            }
        }
    } else {
        for (int pi = 0; pi < h->P; pi++) {
            const int p = f.p_lo + pi;
            const long long total = (long long)nS * h->m * p;
            for (int sg = 1; sg <= f.L; sg++)
                hipLaunchKernelGGL(k_ffa_stage, dim3(mi355_grid_256(h->ctx, total, 32)), dim3(256), 0, st, sg == 1 ? in : plane[sg & 1],
                                   sg == 1 ? in_pitch : slot, plane[(sg + 1) & 1], slot, nS, h->m, p, sg);
            hipLaunchKernelGGL(k_ffa_eval, dim3(mi355_grid_256(h->ctx, (long long)nS * h->m * 64, 32)), dim3(256), 0, st, plane[(f.L + 1) & 1], slot,
                               d_stats, f.S, peaks, profiles, nS, f.L, f.K, p, pi, h->P, f.p_hi);
        }
    }
    MI355_HIP(hipGetLastError());
    rc = h->ws.release(st);
    if (rc) return rc;
    return h->stats.used(st);  // this version of the statistics may be released behind these launches
}

int ffa_args(const mi355_ffa *h, const void *in, long long in_pitch, const void *peaks, const void *profiles)
{
    MI355_REQUIRE(in && peaks, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, "in must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(peaks) & 7u) == 0, "peaks must be 8-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(profiles) & 3u) == 0, "profiles must be 4-byte aligned");
    MI355_REQUIRE(in_pitch >= h->N, "in_pitch is below N = 2^log2_rows p_hi");
    const long long S = h->f.S, rec = (long long)h->P * h->m;
    if (in_pitch > kFfaMaxBytes / (4 * S) || (profiles && rec * h->f.p_hi > kFfaMaxBytes / (4 * S))) {
        mi355_set_error("clPeriodSearch: %lld series of pitch %lld, %lld profiles of %d floats per series (the limit is 2^40 bytes per buffer)", S, in_pitch,
                        rec, h->f.p_hi);
        return MI355_ERR_UNSUPPORTED;
    }
    const long long ib = 4 * ((S - 1) * in_pitch + h->N), pb = 8 * S * rec, fb = 4 * S * rec * h->f.p_hi;
    MI355_REQUIRE(!mi355_overlap(in, ib, peaks, pb), "clPeriodSearch does not work in place: in and peaks overlap");
    if (profiles) {
        MI355_REQUIRE(!mi355_overlap(in, ib, profiles, fb), "in and profiles overlap");
        MI355_REQUIRE(!mi355_overlap(peaks, pb, profiles, fb), "peaks and profiles overlap");
    }
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_ffa_plan(int num_series, int p_lo, int p_hi, int log2_rows, int num_widths, long long *in_floats_per_series,
                              long long *records_per_series, long long *profile_floats_per_series, long long *scratch_bytes)
{
    if (in_floats_per_series) *in_floats_per_series = 0;
    if (records_per_series) *records_per_series = 0;
    if (profile_floats_per_series) *profile_floats_per_series = 0;
    if (scratch_bytes) *scratch_bytes = 0;
    const FfaShape f = {num_series, p_lo, p_hi, log2_rows, num_widths};
    const int rc = ffa_check(f);
    if (rc) return rc;
    const long long m = 1ll << f.L, P = f.p_hi - f.p_lo + 1;
    if (in_floats_per_series) *in_floats_per_series = m * f.p_hi;
    if (records_per_series) *records_per_series = P * m;
    if (profile_floats_per_series) *profile_floats_per_series = P * m * f.p_hi;
    if (scratch_bytes) *scratch_bytes = ffa_scratch_bytes(f);
    return MI355_OK;
}

extern "C" int mi355_ffa_create(mi355_ctx *ctx, int num_series, int p_lo, int p_hi, int log2_rows, int num_widths, const float *mean,
                                const float *inv_sigma, mi355_ffa **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    const FfaShape f = {num_series, p_lo, p_hi, log2_rows, num_widths};
    int rc = ffa_check(f);
    if (rc) return rc;
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_ffa *h = new (std::nothrow) mi355_ffa();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->f = f; h->m = 1 << f.L; h->P = f.p_hi - f.p_lo + 1; h->N = (long long)h->m * f.p_hi;
    ffa_plan(h);
    h->stats.init((size_t)f.S, mean, inv_sigma, "mi355_ffa: statistics");
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_ffa_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = h->stats.publish(ctx);
        if (rc == MI355_OK) rc = h->ws.acquire((size_t)ffa_scratch_bytes(f), ctx->stream[0]);
    }
    if (rc) { mi355_ffa_destroy(h); return rc; }
    ffa_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clPeriodSearch: %d series, base periods %d..%d, 2^%d rows, %d widths: %s", f.S, f.p_lo, f.p_hi, f.L, f.K,
              h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_ffa_destroy(mi355_ffa *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)h->ws.wait();
    h->ws.destroy();
    h->stats.release();
    h->d_in.release();
    h->d_out.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_ffa_set_stats(mi355_ffa *h, const float *mean, const float *inv_sigma)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(mean && inv_sigma, "mean or inv_sigma is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return h->stats.set(h->ctx, mean, inv_sigma);
}

extern "C" int mi355_ffa_get_stats(const mi355_ffa *h, float *mean, float *inv_sigma, long long cap_entries)
{
    MI355_REQUIRE(h && mean && inv_sigma, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_ffa *>(h)->lock);
    MI355_REQUIRE(cap_entries >= (long long)h->f.S, "out too small");
    h->stats.get(mean, inv_sigma);
    return MI355_OK;
}

extern "C" int mi355_ffa_set_generic(mi355_ffa *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    ffa_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_ffa_route(const mi355_ffa *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_ffa_work_dev(mi355_ffa *h, const void *in, long long in_pitch, void *peaks, void *profiles, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = ffa_args(h, in, in_pitch, peaks, profiles);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return ffa_launch(h, 0, h->f.S, (const float *)in, in_pitch, (uint2 *)peaks, (float *)profiles, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_ffa_work(mi355_ffa *h, const void *in, long long in_pitch, void *peaks, void *profiles)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = ffa_args(h, in, in_pitch, peaks, profiles);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole series; the records and the profiles of a piece lie behind one another in d_out
    const long long S = h->f.S, N = h->N, rec = (long long)h->P * h->m;
    const long long peak_bytes = 8 * rec, prof_bytes = profiles ? 4 * rec * h->f.p_hi : 0;
    const long long piece = mi355_piece_units(kFfaHostBytes / (4 * N), S);
    if ((rc = h->d_in.reserve((size_t)(4 * N * piece)))) return rc;
    if ((rc = h->d_out.reserve((size_t)(piece * (peak_bytes + prof_bytes))))) return rc;
    char *d_peaks = (char *)h->d_out.get(), *d_prof = d_peaks + piece * peak_bytes;
    // the device copy of the profiles starts as the caller's: the floats j >= p of a row are never written
    return mi355_pageable_run(h->ctx, S, piece, [&](long long s0, long long ns, hipStream_t st) -> int {
        MI355_HIP(hipMemcpy2DAsync(h->d_in.get(), (size_t)(4 * N), (const float *)in + s0 * in_pitch, (size_t)(4 * in_pitch), (size_t)(4 * N), (size_t)ns,
                                   hipMemcpyHostToDevice, st));
        if (profiles)
            MI355_HIP(hipMemcpyAsync(d_prof, (const char *)profiles + s0 * prof_bytes, (size_t)(ns * prof_bytes), hipMemcpyHostToDevice, st));
        const int lrc = ffa_launch(h, (int)s0, (int)ns, (const float *)h->d_in.get(), N, (uint2 *)d_peaks, profiles ? (float *)d_prof : nullptr, st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)peaks + s0 * peak_bytes, d_peaks, (size_t)(ns * peak_bytes), hipMemcpyDeviceToHost, st));
        if (profiles) MI355_HIP(hipMemcpyAsync((char *)profiles + s0 * prof_bytes, d_prof, (size_t)(ns * prof_bytes), hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
}

// host only: sh(i, r) = sum over stages s of bit_(s-1)(r) (((i >> (L - s)) + 1) >> 1)
extern "C" long long mi355_ffa_shift(int log2_rows, int i, int r)
{
    const int L = log2_rows;
    if (L < 1 || L > kFfaMaxL || i < 0 || r < 0 || i >= (1 << L) || r >= (1 << L)) return MI355_ERR_INVALID_ARG;
    long long sh = 0;
    for (int s = 1; s <= L; s++)
        if ((r >> (s - 1)) & 1) sh += ((i >> (L - s)) + 1) >> 1;
    return sh;
}

// host only: the period of trial (p, i) in seconds, (p + i / (2^L - 1)) tsamp; NaN for arguments outside the ranges
extern "C" double mi355_ffa_period(int p, int log2_rows, int i, double tsamp_s)
{
    const int L = log2_rows;
    if (L < 1 || L > kFfaMaxL || p < kFfaMinP || p > kFfaMaxP || i < 0 || i >= (1 << L) || !(tsamp_s > 0.0) || !std::isfinite(tsamp_s)) return NAN;
    return ((double)p + (double)i / (double)((1 << L) - 1)) * tsamp_s;
}
