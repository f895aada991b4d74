// clXCorrelate: time-domain lag-search correlator (reference lib/clXCorrelate_impl.cc).
// Per frame of N samples and per signal s >= 1 (x = input 0, y = input s, both after the magnitude step :915 for complex items):
//     c(shift) = sum_j x[j+shift] y[j]                    over 0 <= j < N, 0 <= j+shift < N          (kernel :851-899)
//     corr[g]  = c / sqrt(sum x^2 * sum y^2)             both energies over exactly the overlapping samples, g = shift + M
//     corr[g]  = -2                                      when that energy product is 0 (no overlap included)
// then the maximum of corr[0 .. 2M) and its lag g - M (find_max :1014-1045; ties -> lowest g, non-finite entries never win).
//
// Two launches per call:
//   k_xtd_corr   the dot products as window-matrix x Toeplitz-matrix products on v_mfma_f32_16x16x4_f32 (the form of k_fir_mfma,
//                filter.hip): for a tile of 256 lags g = g0 + 16 i + jj and reduction index k,
//                    D[i][jj] = sum_k A[i][k] B[k][jj],   A[i][k] = x[16 i + k],   B[k][jj] = y[M - g0 + k - jj]
//                (zero outside [0, N)); k runs over [-240, N), so every row i sees every t = 16 i + k in [0, N) exactly once.
//                The k axis is cut into chunks of U (a unit = one chunk x one block of 2048 lags); each unit writes its partial
//                tile to a workspace.  Inside a unit the fp32 accumulators are folded into float64 every 2048 values of k, so
//                the fp32 chains stay 512 MFMA steps long whatever N is.  Sub-chunks whose x or y window holds no sample of
//                the frame (lags without overlap) are skipped.  Workgroups 0 and 1 of every (frame, signal) instead build the
//                float64 energy tables of x and y (below).
//   k_xtd_reduce one workgroup per (frame, signal): sums the partial tiles in chunk order (float64), normalises, writes the curve
//                if asked, and takes the argmax.
// The split (U, chunk count) depends only on (N, M), so a batch of frames equals frame-by-frame calls bit for bit.
//
// Energies: every overlap is a prefix [0, L) or a suffix [p, N) of a frame with L > N - M or p < M, so per input only
// suf[p] = sum_{t >= p} v^2 (p = 0..M) and pre[L] = sum_{t < L} v^2 (L = N-M..N) are needed.  They are float64 sums taken from the
// start (prefix) and from the end (suffix) separately, so a run of zeros gives exactly 0 and hence exactly -2.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "common.h"

namespace {

constexpr int kTdMaxInputs = 32;
constexpr int kTdThreads = 256;             // 4 waves
constexpr int kTdLB = 2048;                 // lags per unit: 4 waves x 2 tiles x 256
constexpr int kTdKPad = 240;                // k starts at -240: row 15 of a tile reaches t = 0
constexpr int kTdSub = 2048;                // values of k per LDS fill (and per fp32 chain)
constexpr int kTdRedThreads = 512;
constexpr size_t kTdWsCap = (size_t)256 << 20;  // workspace per launch pair (more (frame, signal) pairs: several launch pairs)

typedef float v4f __attribute__((ext_vector_type(4)));

struct TdIn {
    const void *in[kTdMaxInputs];
};

__host__ __device__ constexpr int td_pad(int n) { return n + ((n >> 4) << 1); }  // 16 values -> 18 slots (k_fir_mfma's A layout)

template <bool CPLX>
__device__ __forceinline__ float td_val(const void *p, long long i)
{
    if constexpr (CPLX) {
        const float2 z = ((const float2 *)p)[i];
        return sqrtf(fmaf(z.x, z.x, z.y * z.y));  // ComplexToMag, :915
    } else {
        return ((const float *)p)[i];
    }
}

// energy tables of one input frame v[0, N): T[p] = suf[p] (p = 0..M), T[M + 1 + i] = pre[N - M + i] (i = 0..M)
template <bool CPLX>
__device__ void td_energy(const void *src, int N, int M, double *__restrict__ T, double *red)
{
    const int tid = threadIdx.x;
    const int S = (N + kTdThreads - 1) / kTdThreads;
    const int s0 = tid * S < N ? tid * S : N, s1 = s0 + S < N ? s0 + S : N;
    // (every walk loads 8 values -- clamped, in-segment indices -- before it adds them in order: one memory latency per 8 samples)
    double tot = 0.0;
    for (int t8 = s0; t8 < s1; t8 += 8) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = td_val<CPLX>(src, t8 + q < s1 ? t8 + q : s1 - 1);
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (t8 + q < s1) tot += (double)v[q] * v[q];
    }
    red[tid] = tot;
    __syncthreads();
    double before = 0.0, after = 0.0;  // sums of the segments before / after this thread's, in a fixed order
    for (int j = 0; j < tid; j++) before += red[j];
    for (int j = kTdThreads - 1; j > tid; j--) after += red[j];
    // prefix sums, L in [max(0, N - M), N]
    const int lo = N - M > 0 ? N - M : 0;
    if (s1 > s0 && s1 > lo) {
        double run = before;
        for (int t8 = s0; t8 < s1; t8 += 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = td_val<CPLX>(src, t8 + q < s1 ? t8 + q : s1 - 1);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int t = t8 + q;
                if (t < s1) {
                    if (t >= lo) T[M + 1 + (t - (N - M))] = run;
                    run += (double)v[q] * v[q];
                }
            }
        }
        if (s1 == N) T[M + 1 + M] = run;
    }
    // suffix sums, p in [0, min(M, N - 1)]
    if (s1 > s0 && s0 <= M) {
        double run = after;
        for (int t8 = s1 - 1; t8 >= s0; t8 -= 8) {
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = td_val<CPLX>(src, t8 - q >= s0 ? t8 - q : s0);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int t = t8 - q;
                if (t >= s0) {
                    run += (double)v[q] * v[q];
                    if (t <= M) T[t] = run;
                }
            }
        }
    }
    // empty overlaps: suf[p] for p >= N, pre[L] for L <= 0
    for (int p = N + tid; p <= M; p += kTdThreads) T[p] = 0.0;
    for (int i = tid; i <= M && N - M + i <= 0; i += kTdThreads) T[M + 1 + i] = 0.0;
}

// dst[i] (padded slots if PAD) = v[base + i] for i < count, 0 outside the frame.  Every load reads a clamped, in-frame index and is
// issued unconditionally, 4 per thread at a time (conditional loads were issued and waited for one by one); the select follows.
template <bool CPLX>
__device__ __forceinline__ void td_stage(float *dst, bool pad, const void *src, long long base, int count, int N)
{
    for (int i0 = threadIdx.x; i0 < count; i0 += 4 * kTdThreads) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const long long t = base + i0 + q * kTdThreads;
            v[q] = td_val<CPLX>(src, t < 0 ? 0 : (t >= N ? N - 1 : t));
            if (t < 0 || t >= N) v[q] = 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = i0 + q * kTdThreads;
            if (i < count) dst[pad ? td_pad(i) : i] = v[q];
        }
    }
}

// grid: x = 2 + nlb * nch (x 0 / 1: energy tables of x / y), y = (frame, signal) pairs of this launch
template <bool CPLX>
__global__ __launch_bounds__(kTdThreads, 2) void k_xtd_corr(TdIn a, int nsig, int N, int M, int U, int nch, long long pair0,
                                                           float *__restrict__ P, double *__restrict__ E)
{
    __shared__ __attribute__((aligned(16))) float xs[td_pad(kTdSub + kTdKPad) + 4];
    __shared__ __attribute__((aligned(16))) float ys[kTdSub + kTdLB];
    const long long pair = pair0 + blockIdx.y;
    const int f = (int)(pair / nsig), s = 1 + (int)(pair % nsig);
    const long long foff = (long long)f * N;
    const size_t isz = CPLX ? 8 : 4;
    const void *xsrc = (const char *)a.in[0] + foff * isz;
    const void *ysrc = (const char *)a.in[s] + foff * isz;
    const int L2 = 2 * M;
    if (blockIdx.x < 2) {
        double *T = E + ((size_t)blockIdx.y * 2 + blockIdx.x) * (size_t)(L2 + 2);
        td_energy<CPLX>(blockIdx.x == 0 ? xsrc : ysrc, N, M, T, (double *)ys);
        return;
    }
    const int unit = blockIdx.x - 2, lb = unit / nch, ch = unit % nch;
    const int gb = lb * kTdLB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    const int tile0 = wave * 2;                             // this wave's tiles: lags gb + 256 * (tile0 + b) + [0, 256)
    const bool busy = gb + 256 * tile0 < L2;               // (wave-uniform)
    double dacc[2][4];
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) dacc[b][r] = 0.0;
    const int sub = U < kTdSub ? U : kTdSub;
    const long long k0 = -(long long)kTdKPad + (long long)ch * U;
    for (int sc = 0; sc < U; sc += sub) {
        const long long kA = k0 + sc;
        // x window: t in [kA, kA + sub + 240); y window: [kA + M - gb - 2047, ... + sub + 2048)
        const long long ybase = kA + M - gb - (kTdLB - 1);
        if (kA >= N || kA + sub + kTdKPad <= 0 || ybase >= N || ybase + sub + kTdLB <= 0) continue;  // (workgroup-uniform)
        __syncthreads();  // the previous sub-chunk's operand reads are done
        td_stage<CPLX>(xs, true, xsrc, kA, sub + kTdKPad, N);
        td_stage<CPLX>(ys, false, ysrc, ybase, sub + kTdLB, N);
        __syncthreads();
        if (!busy) continue;
        v4f acc0 = (v4f){0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        // A[row c][k = 4 kk + g] = xs[16 c + 4 kk + g]; B_b[k][col c] = ys[2047 - 256 (tile0 + b) + 4 kk + g - c]
        const float *xa = xs;
        const int xi0 = 16 * c + g;
        const float *yb0 = ys + (kTdLB - 1 - 256 * tile0 + g - c);
        const float *yb1 = yb0 - 256;
        for (int k8 = 0; k8 < sub / 4; k8 += 8) {  // (sub / 4 is a multiple of 64)
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int kk = k8 + q;
                const float av = xa[td_pad(xi0 + 4 * kk)];
                const float b0 = yb0[4 * kk], b1 = yb1[4 * kk];
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            dacc[0][r] += (double)acc0[r];
            dacc[1][r] += (double)acc1[r];
        }
    }
    if (!busy) return;
    // D[row = 4 g + r][col = c] -> lag g0 + 16 row + c
    float *out = P + ((size_t)blockIdx.y * nch + ch) * (size_t)L2;
#pragma unroll
    for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int lag = gb + 256 * (tile0 + b) + 16 * (4 * g + r) + c;
            if (lag < L2) out[lag] = (float)dacc[b][r];
        }
}

__global__ __launch_bounds__(kTdRedThreads) void k_xtd_reduce(int nsig, int N, int M, int nch, long long pair0, const float *__restrict__ P,
                                                              const double *__restrict__ E, float *__restrict__ corr, int *__restrict__ lags,
                                                              float *__restrict__ curves)
{
    __shared__ float bv[kTdRedThreads];
    __shared__ int bg[kTdRedThreads];
    const long long pair = pair0 + blockIdx.x;
    const int L2 = 2 * M, tid = threadIdx.x;
    const float *p = P + (size_t)blockIdx.x * nch * (size_t)L2;
    const double *Tx = E + (size_t)blockIdx.x * 2 * (size_t)(L2 + 2), *Ty = Tx + (L2 + 2);
    float best = 0.f;
    int bestg = -1;  // -1: no finite entry yet
    for (int gi = tid; gi < L2; gi += kTdRedThreads) {
        double cxy = 0.0;
        for (int c8 = 0; c8 < nch; c8 += 8) {  // 8 loads in flight, then the adds in chunk order
            float v[8];
#pragma unroll
            for (int q = 0; q < 8; q++) v[q] = p[(size_t)(c8 + q < nch ? c8 + q : nch - 1) * L2 + gi];
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (c8 + q < nch) cxy += (double)v[q];
        }
        const int shift = gi - M;
        double ex, ey;
        if (shift >= 0) { ex = Tx[shift]; ey = Ty[M + 1 + (M - shift)]; }
        else { ex = Tx[M + 1 + (M + shift)]; ey = Ty[-shift]; }
        const double den = ex * ey;
        const float v = den != 0.0 ? (float)(cxy / sqrt(den)) : -2.0f;
        if (curves) curves[(size_t)pair * L2 + gi] = v;
        if (isfinite(v) && (bestg < 0 || v > best)) { best = v; bestg = gi; }
    }
    bv[tid] = best;
    bg[tid] = bestg;
    __syncthreads();
    for (int w = kTdRedThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            const float v2 = bv[tid + w];
            const int g2 = bg[tid + w], g1 = bg[tid];
            if (g2 >= 0 && (g1 < 0 || v2 > bv[tid] || (v2 == bv[tid] && g2 < g1))) { bv[tid] = v2; bg[tid] = g2; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        corr[pair] = bg[0] >= 0 ? bv[0] : __builtin_nanf("");
        lags[pair] = (bg[0] >= 0 ? bg[0] : 0) - M;
    }
}

}  // namespace

struct mi355_xcorr_td {
    mi355_ctx *ctx = nullptr;
    int num_inputs = 0, n = 0, max_shift = 0, cplx = 0, isz = 0;
    int u = 0, nch = 0, nlb = 0;
    // workspace of the launches (partial tiles, energy tables); calls on other streams wait for ws_free
    void *d_ws = nullptr;
    size_t ws_bytes = 0;
    hipEvent_t ws_free = nullptr;
    std::mutex ws_lock;
    // host path: the handle's own stream, one pinned region for all inputs, one for the results
    hipStream_t st = nullptr;
    void *h_in = nullptr, *d_in = nullptr, *h_out = nullptr, *d_out = nullptr;
    hipEvent_t done = nullptr;
    int pending = 0;
};

namespace {

size_t td_pair_bytes(const mi355_xcorr_td *h)
{
    return (size_t)h->nch * 2 * (size_t)h->max_shift * 4 + 2 * (2 * (size_t)h->max_shift + 2) * 8;
}

int td_launch(mi355_xcorr_td *h, int nframes, const void *const *d_inputs, float *corr, int *lags, float *curves, hipStream_t st)
{
    const int nsig = h->num_inputs - 1, M = h->max_shift, N = h->n;
    TdIn a{};
    for (int k = 0; k < h->num_inputs; k++) a.in[k] = d_inputs[k];
    const long long pairs = (long long)nframes * nsig;
    const size_t per = td_pair_bytes(h);
    long long group = (long long)(kTdWsCap / per);
    if (group < 1) group = 1;
    if (group > 65535) group = 65535;
    if (group > pairs) group = pairs;
    std::lock_guard<std::mutex> g(h->ws_lock);
    const size_t need = (size_t)group * per;
    if (need > h->ws_bytes) {
        MI355_HIP(hipEventSynchronize(h->ws_free));
        if (h->d_ws) (void)hipFree(h->d_ws);
        h->d_ws = nullptr;
        h->ws_bytes = 0;
        MI355_HIP(hipMalloc(&h->d_ws, need));
        h->ws_bytes = need;
    }
    MI355_HIP(hipStreamWaitEvent(st, h->ws_free, 0));  // an earlier call on another stream may still use the workspace
    float *P = (float *)h->d_ws;
    for (long long p0 = 0; p0 < pairs; p0 += group) {
        const int np = (int)(pairs - p0 < group ? pairs - p0 : group);
        double *E = (double *)((char *)h->d_ws + (size_t)np * h->nch * 2 * (size_t)M * 4);
        const dim3 grid((unsigned)(2 + h->nlb * h->nch), (unsigned)np);
        if (h->cplx)
            hipLaunchKernelGGL((k_xtd_corr<true>), grid, dim3(kTdThreads), 0, st, a, nsig, N, M, h->u, h->nch, p0, P, E);
        else
            hipLaunchKernelGGL((k_xtd_corr<false>), grid, dim3(kTdThreads), 0, st, a, nsig, N, M, h->u, h->nch, p0, P, E);
        MI355_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_xtd_reduce, dim3((unsigned)np), dim3(kTdRedThreads), 0, st, nsig, N, M, h->nch, p0, (const float *)P,
                           (const double *)E, corr, lags, curves);
        MI355_HIP(hipGetLastError());
    }
    MI355_HIP(hipEventRecord(h->ws_free, st));
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_xcorr_td_plan(int signal_length, int max_search_index, int *max_shift)
{
    MI355_REQUIRE(max_shift != nullptr, "NULL argument");
    *max_shift = 0;
    if (signal_length < 2 || signal_length > (1 << 24)) {
        mi355_set_error("signal_length %d not supported (2 .. 16777216)", signal_length);
        return MI355_ERR_UNSUPPORTED;
    }
    // the reference exit(1)s on odd values (lib/clXCorrelate_impl.cc:716-724)
    MI355_REQUIRE(signal_length % 2 == 0, "signal_length must be a multiple of 2");
    MI355_REQUIRE(max_search_index % 2 <= 0, "max_search_index must be a multiple of 2");  // (as there: a negative one takes the 0.7 rule)
    long long m = max_search_index;
    if (m <= 0) {  // :728-734
        m = (int)(0.7 * (float)signal_length);
        if (m % 2) m += 1;
    }
    if (m > (1 << 24)) {
        mi355_set_error("max_search_index %lld not supported (the effective max shift is at most 16777216)", m);
        return MI355_ERR_UNSUPPORTED;
    }
    long long p2 = 1;  // :737-744, round up to a power of two
    while (p2 < m) p2 <<= 1;
    *max_shift = (int)p2;
    return MI355_OK;
}

extern "C" int mi355_xcorr_td_create(mi355_ctx *ctx, int num_inputs, int signal_length, int data_type, int data_size,
                                     int max_search_index, mi355_xcorr_td **out)
{
    MI355_REQUIRE(ctx && out, "NULL argument");
    *out = nullptr;
    if (num_inputs < 2 || num_inputs > kTdMaxInputs) {
        mi355_set_error("num_inputs %d not supported (2 .. %d)", num_inputs, kTdMaxInputs);
        return num_inputs < 2 ? MI355_ERR_INVALID_ARG : MI355_ERR_UNSUPPORTED;
    }
    if (data_type != MI355_DTYPE_COMPLEX && data_type != MI355_DTYPE_FLOAT) {
        mi355_set_error("clXCorrelate data_type %d not supported (1 = complex, 2 = float)", data_type);
        return MI355_ERR_UNSUPPORTED;
    }
    MI355_REQUIRE((size_t)data_size == mi355_dtype_size(data_type), "data_size does not match data_type (8 for complex, 4 for float)");
    int m = 0;
    int rc = mi355_xcorr_td_plan(signal_length, max_search_index, &m);
    if (rc) return rc;
    mi355_xcorr_td *h = new (std::nothrow) mi355_xcorr_td();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->num_inputs = num_inputs; h->n = signal_length; h->max_shift = m;
    h->cplx = data_type == MI355_DTYPE_COMPLEX; h->isz = data_size;
    // the split depends on (N, M) only: blocks of 2048 lags, chunks of U values of k (a power of two >= 256), as many as keep
    // the units of one (frame, signal) at most 512 and its partial tiles within 16 MiB (or one chunk)
    const long long kspan = (long long)signal_length + kTdKPad, lags = 2LL * m;
    h->nlb = (int)((lags + kTdLB - 1) / kTdLB);
    long long u = 256;
    auto chunks = [&](long long uu) { return (kspan + uu - 1) / uu; };
    while ((h->nlb * chunks(u) > 512 || (chunks(u) > 1 && chunks(u) * lags > (4LL << 20))) && u < kspan) u <<= 1;
    h->u = (int)u;
    h->nch = (int)chunks(u);
    auto fail = [&](int code) {
        (void)mi355_xcorr_td_destroy(h);
        return code;
    };
    if (hipSetDevice(ctx->device) != hipSuccess) { mi355_set_error("hipSetDevice failed"); return fail(MI355_ERR_HIP); }
    const size_t in_bytes = (size_t)num_inputs * signal_length * data_size, out_bytes = 2 * 4 * (size_t)(num_inputs - 1);
    if (hipEventCreateWithFlags(&h->ws_free, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->done, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
        mi355_set_error("stream / event creation failed");
        return fail(MI355_ERR_HIP);
    }
    if (hipHostMalloc(&h->h_in, in_bytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&h->d_in, in_bytes) != hipSuccess ||
        hipHostMalloc(&h->h_out, out_bytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&h->d_out, out_bytes) != hipSuccess) {
        mi355_set_error("allocation of the staging buffers failed");
        return fail(MI355_ERR_NOMEM);
    }
    if (m != max_search_index && max_search_index > 0)
        mi355_log(ctx, MI355_LOG_INFO, "clXCorrelate: adjusting max shift to %d for power-of-2 boundary", m);
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_xcorr_td_destroy(mi355_xcorr_td *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    if (h->st) (void)hipStreamSynchronize(h->st);  // a pending submission is dropped (the reference's stop())
    if (h->ws_free) (void)hipEventSynchronize(h->ws_free);
    if (h->d_ws) (void)hipFree(h->d_ws);
    if (h->d_in) (void)hipFree(h->d_in);
    if (h->d_out) (void)hipFree(h->d_out);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_out) (void)hipHostFree(h->h_out);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->ws_free) (void)hipEventDestroy(h->ws_free);
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
    return MI355_OK;
}

extern "C" int mi355_xcorr_td_max_shift(const mi355_xcorr_td *h) { return h ? h->max_shift : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_xcorr_td_work_dev(mi355_xcorr_td *h, int nframes, const void *const *d_inputs, float *d_corr, int *d_lags,
                                       float *d_curves, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (nframes <= 0) return MI355_OK;
    MI355_REQUIRE(d_inputs && d_corr && d_lags, "NULL pointer");
    for (int k = 0; k < h->num_inputs; k++) MI355_REQUIRE(d_inputs[k] != nullptr, "NULL input buffer");
    if ((long long)nframes * h->n > (1LL << 40)) { mi355_set_error("work() call too large"); return MI355_ERR_INVALID_ARG; }
    MI355_HIP(hipSetDevice(h->ctx->device));
    return td_launch(h, nframes, d_inputs, d_corr, d_lags, d_curves, mi355_pick_stream(h->ctx, stream));
}

namespace {

// one frame of host inputs -> pinned staging -> ONE H2D copy -> two kernels -> ONE D2H copy of corr and lags; enqueued on h->st
int td_enqueue_host(mi355_xcorr_td *h, const void *const *inputs)
{
    const size_t frame = (size_t)h->n * h->isz;
    for (int k = 0; k < h->num_inputs; k++) MI355_REQUIRE(inputs[k] != nullptr, "NULL input buffer");
    for (int k = 0; k < h->num_inputs; k++) mi355_copy((char *)h->h_in + k * frame, inputs[k], frame);
    MI355_HIP(hipMemcpyAsync(h->d_in, h->h_in, frame * h->num_inputs, hipMemcpyHostToDevice, h->st));
    const void *din[kTdMaxInputs];
    for (int k = 0; k < h->num_inputs; k++) din[k] = (const char *)h->d_in + k * frame;
    const int nsig = h->num_inputs - 1;
    int rc = td_launch(h, 1, din, (float *)h->d_out, (int *)h->d_out + nsig, nullptr, h->st);
    if (rc) return rc;
    MI355_HIP(hipMemcpyAsync(h->h_out, h->d_out, 8 * (size_t)nsig, hipMemcpyDeviceToHost, h->st));
    MI355_HIP(hipEventRecord(h->done, h->st));
    return MI355_OK;
}

void td_collect(mi355_xcorr_td *h, float *corr, int *lags)
{
    const int nsig = h->num_inputs - 1;
    if (corr) memcpy(corr, h->h_out, 4 * (size_t)nsig);
    if (lags) memcpy(lags, (const int *)h->h_out + nsig, 4 * (size_t)nsig);
}

}  // namespace

extern "C" int mi355_xcorr_td_work(mi355_xcorr_td *h, const void *const *inputs, float *corr, int *lags)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(inputs && corr && lags, "NULL pointer");
    if (h->pending) { mi355_set_error("a submission is pending: collect it with mi355_xcorr_td_poll first"); return MI355_ERR_STATE; }
    MI355_HIP(hipSetDevice(h->ctx->device));
    int rc = td_enqueue_host(h, inputs);
    if (rc) return rc;
    MI355_HIP(hipEventSynchronize(h->done));
    td_collect(h, corr, lags);
    return MI355_OK;
}

extern "C" int mi355_xcorr_td_submit(mi355_xcorr_td *h, const void *const *inputs)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(inputs != nullptr, "NULL pointer");
    if (h->pending) { mi355_set_error("a submission is pending: collect it with mi355_xcorr_td_poll first"); return MI355_ERR_STATE; }
    MI355_HIP(hipSetDevice(h->ctx->device));
    int rc = td_enqueue_host(h, inputs);
    if (rc) return rc;
    h->pending = 1;
    return MI355_OK;
}

extern "C" int mi355_xcorr_td_poll(mi355_xcorr_td *h, float *corr, int *lags)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (!h->pending) { mi355_set_error("nothing submitted"); return MI355_ERR_STATE; }
    const hipError_t e = hipEventQuery(h->done);
    if (e == hipErrorNotReady) return 0;
    MI355_HIP(e);
    td_collect(h, corr, lags);
    h->pending = 0;
    return 1;
}

extern "C" int mi355_xcorr_td_wait(mi355_xcorr_td *h)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (h->pending) MI355_HIP(hipEventSynchronize(h->done));
    return MI355_OK;
}
