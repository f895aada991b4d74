// clPowerSpectrum: window + forward DFT + |X|^2 + average over K frames (+ dB) as gfx950 HIP kernels -- the periodogram estimator
// (Bartlett H = N, Welch H < N, logpwrfft's frame-rate decimation H > N).  The contract is restated in include/mi355_clenabled.h; the
// reference module has no such block.
//
//     P_s[b] = scale / K * sum_{k < K} | DFT_N( w .* x[(s K + k) H + (0 .. N)) )[b] |^2            [fftshift] [10 log10]
//
// Two routes, named by mi355_pspec_route():
//
// fused pow2     k_pspec<N>, N = 16 .. 4096.  256 threads, a frame group = 4096 / N frames = the 4096 points of one fft_core transform in the
//                16-points-per-thread layout, exactly clFFT's k_fft up to the last butterfly.  One workgroup owns one (spectrum, chunk of C
//                frames) pair: it loads group after group at frame stride H (the next group's loads in flight during the transform), and
//                adds re^2 + im^2 of its 16 values to 16 accumulators -- no store per frame at all.  At the end of the chunk the per-frame-slot
//                partials meet in LDS and are added in a fixed order.  K <= C: the workgroup finishes (scale / K, shift, log) and stores N
//                floats.  K > C: it stores its N partial sums into a workspace of the handle and k_pspec_finish adds the ceil(K / C) partials
//                of a bin in index order.  C = max(64, 16 groups): the partials are 1 / (2 C) <= 0.8 % of the input bytes.
// generic        every other length clFFT takes, and any handle under mi355_pspec_set_generic(h, 1): an internal clFFT handle (window and
//                shift are its own) transforms a bounded batch of frames into a workspace -- gathered first by k_pspec_gather when H != N --
//                and k_pspec_acc adds |X|^2 over the frames of a spectrum, one thread per bin, k ascending.
//
// The partition of K and the order of every sum are functions of (N, K) alone -- never of the number of spectra of the call, of a
// spectrum's place in it or of the device -- and there are no float atomics: any split of a stream into calls at spectrum boundaries,
// at any legal alignment, gives the same bits within a route.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "fft_core.hpp"

namespace {

using namespace fftc;
typedef float f2v __attribute__((ext_vector_type(2)));

constexpr int kPsPts = 4096;                       // points per frame group of the fused route
constexpr long long kPsGenItems = 1ll << 20;       // generic route: transformed values per batch of a spectrum longer than that (8 MiB; one frame when N is larger)
constexpr long long kPsGenSpectra = 4ll << 20;     // generic route: transformed values per batch of whole spectra (32 MiB); a bin's sum is one chain either way
constexpr long long kPsMaxGrid = 1ll << 30;        // workgroups per launch
constexpr long long kPsWsFloats = 16ll << 20;      // fused route, K > C: partial sums per launch (64 MiB) unless one spectrum needs more
constexpr long long kPsHostBytes = 64ll << 20;     // host path: input bytes per staged piece unless one spectrum needs more

__host__ __device__ constexpr int ps_chunk(int n) { return (kPsPts / n) * 16 > 64 ? (kPsPts / n) * 16 : 64; }

struct PsArgs {
    const f2v *in;        // first item of the launch's first spectrum
    float *out;           // K <= C: the spectra (N floats each); K > C: the partial sums, [spectrum][chunk][bin] in natural bin order
    const float *window;  // N floats (all ones when the block has none)
    const c32 *tw;        // exp(-2 pi i k / N)
    long long H;
    int K, C, nchunks, shift, log_output;
    float sk;             // scale / K
};

__device__ __forceinline__ float ps_finish(float sum, float sk, int log_output)
{
    const float p = sum * sk;
    return log_output ? 10.0f * log10f(p) : p;
}

template <int N>
__global__ __launch_bounds__(256, 2) void k_pspec(const PsArgs a)
{
    using G = Geo<N>;
    using P = Plan<N>;
    static_assert(G::TH == 256 && G::PTS == kPsPts, "geometry");
    constexpr int TH = 256, F = G::F, NP = P::NP, R0 = P::radix(0), B0 = N / R0, RL = P::radix(NP - 1), BL = N / RL;
    // N <= 64: consecutive elements per lane, redistributed through a padded LDS image -- as in k_fft
    constexpr bool SMALL = N <= 64;
    constexpr int PAD = B0 > 1 ? B0 : 1;
    constexpr int LDS_SLOTS = SMALL ? kPsPts + F * PAD : kPsPts;
    __shared__ c32 lds[LDS_SLOTS];
    const int tid0 = threadIdx.x;
    const long long s = (long long)blockIdx.x / a.nchunks;
    const int c = (int)((long long)blockIdx.x - s * a.nchunks);
    const int k0 = c * a.C, kend = k0 + a.C < a.K ? k0 + a.C : a.K;  // the chunk's frames: k0 .. kend-1 of spectrum s
    const f2v *base = a.in + (s * a.K + k0) * a.H;

    TwRegs<N> tw;
    load_twiddles<N, false, G>(tw, tid0, a.tw);
    float win[16];
    if constexpr (SMALL) {
        win[0] = a.window[tid0 % N];
    } else {
#pragma unroll
        for (int q = 0; q < 16 / R0; q++) {
            const int j = (tid0 + TH * q) % B0;
#pragma unroll
            for (int r = 0; r < R0; r++) win[q * R0 + r] = a.window[j + r * B0];
        }
    }

    // Raw pass-0 inputs of the group whose first frame is kg: streaming loads, branch free.  A thread whose frame lies past the chunk
    // reads the group's first frame instead (it exists, inside the call's items) and keeps an exact zero.
    auto load = [&](c32 (&v)[16], int kg, int tid) {
        const int left = kend - kg;
        const f2v *gp = base + (long long)(kg - k0) * a.H;
        if constexpr (SMALL) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const unsigned e = (unsigned)(tid + TH * k);
                const int fr = (int)(e / N), pos = (int)(e % N);
                const bool ok = fr < left;
                const f2v x = __builtin_nontemporal_load(gp + (long long)(ok ? fr : 0) * a.H + pos);
                v[k] = ok ? mk(x.x, x.y) : mk(0.f, 0.f);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16 / R0; q++) {
                const int g = tid + TH * q, fr = g / B0;
                const bool ok = (F == 1) || fr < left;
                const f2v *p = gp + (long long)(ok ? fr : 0) * a.H + (g % B0);
#pragma unroll
                for (int r = 0; r < R0; r++) {
                    const f2v x = __builtin_nontemporal_load(p + r * B0);
                    v[q * R0 + r] = ok ? mk(x.x, x.y) : mk(0.f, 0.f);
                }
            }
        }
    };

    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;

    c32 cur[16];
    load(cur, k0, tid0);
    for (int kg = k0; kg < kend; kg += F) {
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        c32 nxt[16];
        if (kg + F < kend) load(nxt, kg + F, tid);
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the transform
        c32 v[16];
        if constexpr (SMALL) {
            const float wv = win[0];
            const int pos = tid % N, fr0 = tid / N;
#pragma unroll
            for (int k = 0; k < 16; k++) lds[(fr0 + k * (TH / N)) * (N + PAD) + pos] = scale(cur[k], wv);
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16 / R0; q++) {
                const int g = tid + TH * q, b = (g / B0) * (N + PAD) + (g % B0);
#pragma unroll
                for (int r = 0; r < R0; r++) v[q * R0 + r] = lds[b + r * B0];
            }
            __syncthreads();  // the transform reuses the LDS in its own layout
        } else {
#pragma unroll
            for (int i = 0; i < 16; i++) v[i] = scale(cur[i], win[i]);
        }
        transform_regs<N, -1, false, G>(v, tw, lds, tid);
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = fmaf(v[i].y, v[i].y, fmaf(v[i].x, v[i].x, acc[i]));
        if constexpr (NP > 1 || SMALL) __syncthreads();  // the last pass' LDS reads finish before the next group's writes
#pragma unroll
        for (int i = 0; i < 16; i++) cur[i] = nxt[i];  // (after the last group: values nobody reads, as in k_fft's prefetch loop)
    }

    // acc[q RL + s] is the sum over the chunk's groups of |X[j + orev(s) BL]|^2 of frame slot fr (g = tid + 256 q, fr = g / BL, j = g % BL):
    // the F slot partials of a bin meet in LDS and are added in slot order (N < 256: 16 slots per thread first, then the 256 / N runs).
    float *red = (float *)lds;  // F N = 4096 floats, then 256 more for the runs
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16 / RL; q++) {
        const int g = tid0 + TH * q, fr = g / BL, j = g % BL;
#pragma unroll
        for (int s2 = 0; s2 < RL; s2++) red[fr * N + j + orev<RL>(s2) * BL] = acc[q * RL + s2];
    }
    __syncthreads();
    const int oxor = a.shift ? N / 2 : 0;
    float *dst = a.out + ((long long)blockIdx.x) * N;  // final: nchunks == 1, blockIdx.x == s
    const bool final_ = a.nchunks == 1;
    if constexpr (N >= 256) {
#pragma unroll
        for (int i = 0; i < N / 256; i++) {
            const int b = tid0 + 256 * i;
            float t = red[b];
#pragma unroll
            for (int fr = 1; fr < F; fr++) t += red[fr * N + b];
            if (final_) dst[b ^ oxor] = ps_finish(t, a.sk, a.log_output);
            else dst[b] = t;
        }
    } else {
        constexpr int SEGS = 256 / N, FPS = F / SEGS;
        static_assert(FPS == 16, "sixteen frame slots per thread");
        const int b = tid0 % N, sg = tid0 / N;
        float t = red[(sg * FPS) * N + b];
#pragma unroll
        for (int fr = 1; fr < FPS; fr++) t += red[(sg * FPS + fr) * N + b];
        red[kPsPts + tid0] = t;  // [sg][b]
        __syncthreads();
        if (tid0 < N) {
            float u = red[kPsPts + tid0];
#pragma unroll
            for (int g2 = 1; g2 < SEGS; g2++) u += red[kPsPts + g2 * N + tid0];
            if (final_) dst[tid0 ^ oxor] = ps_finish(u, a.sk, a.log_output);
            else dst[tid0] = u;
        }
    }
}

// K > C: out[s N + o] from the nchunks partial sums of bin b = o ^ oxor, added in chunk order
__global__ __launch_bounds__(256) void k_pspec_finish(const float *__restrict__ ws, float *__restrict__ out, int N, int nchunks, int oxor, float sk,
                                                      int log_output, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long s = idx / N;
        const int b = (int)(idx - s * N) ^ oxor;
        const float *p = ws + s * nchunks * N + b;
        float t = p[0];
        int c = 1;
        for (; c + 32 <= nchunks; c += 32) {  // 32 loads in flight, the adds in chunk order
            float v[32];
#pragma unroll
            for (int i = 0; i < 32; i++) v[i] = p[(long long)(c + i) * N];
#pragma unroll
            for (int i = 0; i < 32; i++) t += v[i];
        }
        for (; c < nchunks; c++) t += p[(long long)c * N];
        out[idx] = ps_finish(t, sk, log_output);
    }
}

// ---- generic route ------------------------------------------------------------------------------------------------------------
// dst[f N + i] = src[f H + i], f < nfr
__global__ __launch_bounds__(256) void k_pspec_gather(const f2v *__restrict__ src, f2v *__restrict__ dst, int N, long long H, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long f = idx / N;
        dst[idx] = src[f * H + (idx - f * N)];
    }
}

// X: nsp spectra of nfr transformed frames each.  acc (N floats per spectrum) carries the sum from one batch of a spectrum's frames to the
// next: read unless `first`, written unless `last`; `last` writes the finished value to out.  One thread per (spectrum, bin), k ascending.
__global__ __launch_bounds__(256) void k_pspec_acc(const c32 *__restrict__ X, float *__restrict__ acc, float *__restrict__ out, int N, int nfr, int first,
                                                   int last, float sk, int log_output, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long s = idx / N;
        const long long b = idx - s * N;
        const c32 *p = X + s * nfr * N + b;
        float t = first ? 0.f : acc[idx];
        int k = 0;
        for (; k + 16 <= nfr; k += 16) {  // 16 loads in flight, the sum in frame order
            c32 v[16];
#pragma unroll
            for (int i = 0; i < 16; i++) v[i] = p[(long long)(k + i) * N];
#pragma unroll
            for (int i = 0; i < 16; i++) t = fmaf(v[i].y, v[i].y, fmaf(v[i].x, v[i].x, t));
        }
        for (; k < nfr; k++) {
            const c32 v = p[(long long)k * N];
            t = fmaf(v.y, v.y, fmaf(v.x, v.x, t));
        }
        if (last) out[idx] = ps_finish(t, sk, log_output);
        else acc[idx] = t;
    }
}

// what can be told without a device; plan_only: nothing about the window
int ps_check(int N, int K, int H)
{
    MI355_REQUIRE(N >= 1, "fft_size must be >= 1");
    MI355_REQUIRE(K >= 1, "navg must be >= 1");
    MI355_REQUIRE(H >= 1, "hop must be >= 1");
    char why[160];
    if (mi355_fft_plan_text(N, why, (int)sizeof why) != MI355_OK) {
        mi355_set_error("fft size %d %s", N, why);  // clFFT's own words
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

// items of S spectra; false: they do not fit 2^62
bool ps_counts(int N, int K, int H, long long S, long long *nin, long long *nout)
{
    const __int128 lim = (__int128)1 << 62;
    const __int128 i = S == 0 ? 0 : ((__int128)S * K - 1) * H + N, o = (__int128)S * N;
    if (i > lim || o > lim) return false;
    *nin = (long long)i;
    *nout = (long long)o;
    return true;
}

bool ps_fused_size(int N) { return N >= 16 && N <= 4096 && (N & (N - 1)) == 0; }

}  // namespace

struct mi355_pspec {
    mi355_ctx *ctx = nullptr;
    int N = 1, K = 1, H = 1, shift = 0, log_output = 0;
    float scale = 1.f;
    bool has_window = false, force_generic = false;
    std::vector<float> win_host;          // N floats (ones without a window)
    mi355_tables win;                     // fused route: the window, N floats
    void *d_tw = nullptr;                 // fused route: exp(-2 pi i k / N)
    mi355_fft *fft = nullptr;             // generic route, made when first needed (and again after set_window)
    std::string route_name;
    // one workspace per handle (fused K > C: partial sums; generic: gathered frames, transformed frames, carried sums); calls on different
    // streams are ordered on it: the later stream waits for the earlier call's kernels
    DevWorkspace ws;
    DevBuf d_in, d_out;  // host path staging
    std::mutex lock;
};

namespace {

bool ps_is_fused(const mi355_pspec *h) { return ps_fused_size(h->N) && !h->force_generic; }

long long ps_gen_batch(int N)
{
    const long long b = kPsGenItems / N;
    return b < 1 ? 1 : b;
}

void ps_name(mi355_pspec *h)
{
    char name[96];
    if (ps_is_fused(h)) snprintf(name, sizeof name, "fused pow2 N=%d chunk=%d", h->N, ps_chunk(h->N));
    else snprintf(name, sizeof name, "generic N=%d batch=%lld", h->N, ps_gen_batch(h->N));
    h->route_name = name;
}

// caller holds h->lock (or is create) and has set the device
int ps_ensure_fft(mi355_pspec *h)
{
    if (h->fft) return MI355_OK;
    return mi355_fft_create(h->ctx, h->N, MI355_FFT_FORWARD, h->has_window ? h->win_host.data() : nullptr, h->has_window ? h->N : 0, MI355_DTYPE_COMPLEX,
                            1, h->shift, &h->fft);
}

#define PS_SIZES(X) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

int ps_launch_fused(mi355_pspec *h, long long S, const void *in, float *out, hipStream_t st)
{
    const int N = h->N, K = h->K, C = ps_chunk(N);
    const int nchunks = (K + C - 1) / C;
    PsArgs a;
    a.window = (const float *)h->win.current();
    a.tw = (const c32 *)h->d_tw;
    a.H = h->H;
    a.K = K;
    a.C = C;
    a.nchunks = nchunks;
    a.shift = h->shift;
    a.log_output = h->log_output;
    a.sk = (float)((double)h->scale / (double)K);
    long long per = kPsMaxGrid / nchunks;  // spectra per launch
    if (nchunks > 1) {
        long long w = kPsWsFloats / ((long long)nchunks * N);
        if (w < 1) w = 1;
        if (w < per) per = w;
    }
    if (per < 1) {
        mi355_set_error("clPowerSpectrum: navg %d is %d chunks of %d frames, more than one launch holds", K, nchunks, C);
        return MI355_ERR_UNSUPPORTED;
    }
    if (per > S) per = S;
    if (nchunks > 1) {
        const int rc = h->ws.acquire((size_t)per * nchunks * N * sizeof(float), st);
        if (rc) return rc;
    }
    for (long long s0 = 0; s0 < S; s0 += per) {
        const long long n = S - s0 < per ? S - s0 : per;
        a.in = (const f2v *)in + s0 * K * (long long)h->H;
        a.out = nchunks > 1 ? (float *)h->ws.get() : out + s0 * N;
        const unsigned grid = (unsigned)(n * nchunks);
#define X(NN) if (N == NN) hipLaunchKernelGGL((k_pspec<NN>), dim3(grid), dim3(256), 0, st, a);
        PS_SIZES(X)
#undef X
        if (nchunks > 1)
            hipLaunchKernelGGL(k_pspec_finish, dim3(mi355_grid_256(h->ctx, n * N, 32)), dim3(256), 0, st, (const float *)h->ws.get(), out + s0 * N, N, nchunks,
                               h->shift ? N / 2 : 0, a.sk, h->log_output, n * N);
    }
    MI355_HIP(hipGetLastError());
    return nchunks > 1 ? h->ws.release(st) : MI355_OK;
}

int ps_launch_generic(mi355_pspec *h, long long S, const void *in, float *out, hipStream_t st)
{
    int rc = ps_ensure_fft(h);
    if (rc) return rc;
    const int N = h->N, K = h->K;
    const long long H = h->H, B = ps_gen_batch(N);  // frames per batch: a function of N alone
    // frames are gathered when H != N, and at sizes above 4096 points, which clFFT reads sixteen bytes at a time, from a pointer that is not so aligned
    const bool gather = H != N || N > 4096;
    const float sk = (float)((double)h->scale / (double)K);
    // whole spectra per batch: at least one (K N may pass kPsGenSpectra: above 2^20 points B is 1 and K = 1 still comes this way), at most S
    long long per = 0;
    if (K <= B) {
        per = kPsGenSpectra / ((long long)K * N);
        if (per < 1) per = 1;
        if (per > S) per = S;
    }
    const long long nb = K <= B ? K * per : B;     // frames of the largest batch
    // [gathered frames][transformed frames][carried sums]
    const size_t frames_bytes = (size_t)nb * N * 8, acc_bytes = (size_t)N * sizeof(float);
    rc = h->ws.acquire((gather ? 2 : 1) * frames_bytes + acc_bytes, st);
    if (rc) return rc;
    char *ws = (char *)h->ws.get();
    f2v *d_g = (f2v *)ws;
    c32 *d_x = (c32 *)(ws + (gather ? frames_bytes : 0));
    float *d_acc = (float *)(ws + (gather ? 2 : 1) * frames_bytes);
    auto transform = [&](const f2v *src, long long nfr) {
        const void *fin = src;
        if (H != N || (N > 4096 && (reinterpret_cast<uintptr_t>(src) & 15u) != 0)) {
            hipLaunchKernelGGL(k_pspec_gather, dim3(mi355_grid_256(h->ctx, nfr * N, 32)), dim3(256), 0, st, src, d_g, N, H, nfr * N);
            fin = d_g;
        }
        return mi355_fft_work_dev(h->fft, (int)nfr, fin, d_x, (void *)st);
    };
    if (K <= B) {
        for (long long s0 = 0; s0 < S; s0 += per) {
            const long long n = S - s0 < per ? S - s0 : per;
            rc = transform((const f2v *)in + s0 * K * H, n * K);
            if (rc) return rc;
            hipLaunchKernelGGL(k_pspec_acc, dim3(mi355_grid_256(h->ctx, n * N, 32)), dim3(256), 0, st, (const c32 *)d_x, d_acc, out + s0 * N, N, K, 1, 1, sk,
                               h->log_output, n * N);
        }
    } else {
        for (long long s = 0; s < S; s++)
            for (long long f0 = 0; f0 < K; f0 += B) {
                const long long n = K - f0 < B ? K - f0 : B;
                rc = transform((const f2v *)in + (s * K + f0) * H, n);
                if (rc) return rc;
                hipLaunchKernelGGL(k_pspec_acc, dim3(mi355_grid_256(h->ctx, N, 32)), dim3(256), 0, st, (const c32 *)d_x, d_acc, out + s * N, N, (int)n, f0 == 0,
                                   f0 + n == K, sk, h->log_output, (long long)N);
            }
    }
    MI355_HIP(hipGetLastError());
    return h->ws.release(st);
}

// caller holds h->lock and has set the device
int ps_launch(mi355_pspec *h, long long S, const void *in, void *out, hipStream_t st)
{
    return ps_is_fused(h) ? ps_launch_fused(h, S, in, (float *)out, st) : ps_launch_generic(h, S, in, (float *)out, st);
}

int ps_args(const mi355_pspec *h, long long S, const void *in, void *out, long long *nin, long long *nout)
{
    MI355_REQUIRE(S >= 0, "nspectra is negative");
    *nin = *nout = 0;
    if (S == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 7u) == 0, "input must be 8-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, "output must be 4-byte aligned");
    if (!ps_counts(h->N, h->K, h->H, S, nin, nout) || *nin > (1ll << 44) || *nout > (1ll << 44)) {
        mi355_set_error("clPowerSpectrum: %lld spectra of %d x %d points in one call", S, h->K, h->N);
        return MI355_ERR_UNSUPPORTED;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    MI355_REQUIRE(!(a < b + (uintptr_t)*nout * 4 && b < a + (uintptr_t)*nin * 8), "clPowerSpectrum does not work in place: in and out overlap");
    return MI355_OK;
}

// caller holds h->lock (or is create) and has set the device
int ps_upload_window(mi355_pspec *h)
{
    return h->win.publish(h->ctx, h->win_host.data(), (size_t)h->N * sizeof(float), "mi355_pspec: window");
}

}  // namespace

extern "C" int mi355_pspec_plan(int fft_size, int navg, int hop, long long nspectra, long long *ninput_items, long long *noutput_items)
{
    if (ninput_items) *ninput_items = 0;
    if (noutput_items) *noutput_items = 0;
    const int rc = ps_check(fft_size, navg, hop);
    if (rc) return rc;
    MI355_REQUIRE(nspectra >= 0, "nspectra is negative");
    long long nin = 0, nout = 0;
    if (!ps_counts(fft_size, navg, hop, nspectra, &nin, &nout)) {
        mi355_set_error("clPowerSpectrum: %lld spectra of %d x %d points at hop %d: the item counts pass 2^62", nspectra, navg, fft_size, hop);
        return MI355_ERR_UNSUPPORTED;
    }
    if (ninput_items) *ninput_items = nin;
    if (noutput_items) *noutput_items = nout;
    return MI355_OK;
}

extern "C" int mi355_pspec_create(mi355_ctx *ctx, int fft_size, const float *window, int window_len, int navg, int hop, int shift, int log_output,
                                  float scale, mi355_pspec **out)
{
    if (out) *out = nullptr;
    // everything that can be told without a device comes first
    MI355_REQUIRE(fft_size >= 1, "fft_size must be >= 1");
    MI355_REQUIRE(window_len == 0 || window_len == fft_size, "window not the same length as fft_size");
    MI355_REQUIRE(window_len == 0 || window != nullptr, "window is NULL");
    int rc = ps_check(fft_size, navg, hop);
    if (rc) return rc;
    MI355_REQUIRE(ctx && out, "NULL argument");
    mi355_pspec *h = new (std::nothrow) mi355_pspec();
    if (!h) return MI355_ERR_NOMEM;
    const int N = fft_size;
    h->ctx = ctx; h->N = N; h->K = navg; h->H = hop; h->shift = shift ? 1 : 0; h->log_output = log_output ? 1 : 0; h->scale = scale;
    h->has_window = window_len != 0;
    h->win_host.assign((size_t)N, 1.0f);
    if (window_len) memcpy(h->win_host.data(), window, sizeof(float) * (size_t)N);
    ps_name(h);
    auto fail = [&](int code) {
        mi355_pspec_destroy(h);
        return code;
    };
    if (hipSetDevice(ctx->device) != hipSuccess) {
        mi355_set_error("mi355_pspec_create: hipSetDevice failed");
        return fail(MI355_ERR_HIP);
    }
    if (ps_fused_size(N)) {
        std::vector<float> tw((size_t)2 * N);
        for (int k = 0; k < N; k++) {
            const double a = -2.0 * M_PI * (double)k / (double)N;
            tw[2 * k] = (float)cos(a);
            tw[2 * k + 1] = (float)sin(a);
        }
        if (hipMalloc(&h->d_tw, tw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_NOMEM);
        if (mi355_upload(ctx, h->d_tw, tw.data(), tw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_HIP);
        if ((rc = ps_upload_window(h))) return fail(rc);
    } else if ((rc = ps_ensure_fft(h))) {
        return fail(rc);
    }
    mi355_log(ctx, MI355_LOG_INFO, "clPowerSpectrum: %d points, %d frames per spectrum, hop %d, shift %d, dB %d, window %s: %s", N, navg, hop, h->shift,
              h->log_output, window_len ? "given" : "none", h->route_name.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_pspec_destroy(mi355_pspec *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    if (h->fft) (void)mi355_fft_destroy(h->fft);
    h->win.release();
    if (h->d_tw) (void)hipFree(h->d_tw);
    h->ws.destroy();
    for (DevBuf *b : {&h->d_in, &h->d_out}) b->release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_pspec_set_scale(mi355_pspec *h, float scale)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->scale = scale;
    return MI355_OK;
}

extern "C" int mi355_pspec_set_window(mi355_pspec *h, const float *window, int window_len)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(window_len == 0 || window_len == h->N, "window not the same length as fft_size");
    MI355_REQUIRE(window_len == 0 || window != nullptr, "window is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    h->has_window = window_len != 0;
    h->win_host.assign((size_t)h->N, 1.0f);
    if (window_len) memcpy(h->win_host.data(), window, sizeof(float) * (size_t)h->N);
    if (h->fft) {  // the internal clFFT carries its window: a new one is made at the next generic call (its kernels in flight end first)
        if (const int rc = h->ws.wait()) return rc;
        (void)mi355_fft_destroy(h->fft);
        h->fft = nullptr;
    }
    if (h->win.current()) return ps_upload_window(h);
    return MI355_OK;
}

extern "C" int mi355_pspec_set_generic(mi355_pspec *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->force_generic = on != 0;
    ps_name(h);
    return MI355_OK;
}

extern "C" int mi355_pspec_fft_size(const mi355_pspec *h) { return h ? h->N : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_pspec_navg(const mi355_pspec *h) { return h ? h->K : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_pspec_hop(const mi355_pspec *h) { return h ? h->H : MI355_ERR_INVALID_ARG; }
// valid until the next set_generic or destroy of this handle
extern "C" const char *mi355_pspec_route(const mi355_pspec *h) { return h ? h->route_name.c_str() : ""; }

extern "C" int mi355_pspec_work_dev(mi355_pspec *h, long long nspectra, const void *in, void *out, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    long long nin, nout;
    const int rc = ps_args(h, nspectra, in, out, &nin, &nout);
    if (rc || nspectra == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = mi355_pick_stream(h->ctx, stream);
    const int rc2 = ps_launch(h, nspectra, in, out, st);
    return rc2 || !ps_is_fused(h) ? rc2 : h->win.used(st);  // this window may be released behind this launch
}

extern "C" int mi355_pspec_work(mi355_pspec *h, long long nspectra, const void *in, void *out)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    long long nin, nout;
    int rc = ps_args(h, nspectra, in, out, &nin, &nout);
    if (rc || nspectra == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole spectra; a piece re-sends the max(N - H, 0) items it shares with the piece before
    const long long per_spec = (long long)h->K * h->H * 8;
    const long long piece = mi355_piece_units(kPsHostBytes / per_spec, nspectra);
    long long pin, pout;
    (void)ps_counts(h->N, h->K, h->H, piece, &pin, &pout);
    if ((rc = h->d_in.reserve((size_t)pin * 8))) return rc;
    if ((rc = h->d_out.reserve((size_t)pout * 4))) return rc;
    return mi355_pageable_run(h->ctx, nspectra, piece, [&](long long s0, long long n, hipStream_t st) -> int {
        (void)ps_counts(h->N, h->K, h->H, n, &pin, &pout);
        MI355_HIP(hipMemcpyAsync(h->d_in.get(), (const char *)in + s0 * per_spec, (size_t)pin * 8, hipMemcpyHostToDevice, st));
        const int lrc = ps_launch(h, n, h->d_in.get(), h->d_out.get(), st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + s0 * h->N * 4, h->d_out.get(), (size_t)pout * 4, hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
}
