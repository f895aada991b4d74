// clFEngine: polyphase filter bank + forward DFT + gain + int8 quantisation into the X-engine's frames as gfx950 HIP kernels -- the
// F-engine in front of clXEngine and clBeamformer.  The contract is restated in include/mi355_clenabled.h; the reference module has no
// such block.  R = S npol complex64 streams (r = s npol + p), F channels, P taps per channel (P F real prototype taps h):
//
//     z[n] = sum_{p < P} h[p F + n] x_r[(t + p) F + n]                 the critically sampled analysis bank: hop F, window P F
//     X[f] = sum_n z[n] exp(-j 2 pi f n / F)
//     out[t][s][f'][p] = int8 { sat(rint(gain[r][f] X[f].re)), sat(rint(gain[r][f] X[f].im)) },      f' = shift ? (f + F / 2) mod F : f
// (for a power of two that is f ^ (F / 2), which is what the fused kernel computes)
//
// rint is round half to even (v_rndne_f32), sat clamps to -127 .. 127, a NaN becomes 0; every component that saturated or was NaN adds
// one to the clip counter of its input (integer atomics: the totals are exact whatever the split into calls).
//
// Two routes, named by mi355_fengine_route():
//
// fused          k_fengine<F, npol>, F = 16 .. 4096 a power of two, P <= 16.  256 threads; a frame group = 4096 / F consecutive frames of
//                one input = the 4096 points of one fft_core transform in the 16-points-per-thread layout, loaded as in k_pspec.  A
//                workgroup owns (station, run of frame groups) and, with npol = 2, both polarisations of the station.  Arm 0 of the next
//                group is in flight during the transform; arms 1 .. P-1 are multiply-adds on the 16 points a thread owns, their items and
//                taps read again through L1 / L2 (the overlapping frames of a group are read by the same workgroup within one step).  The
//                epilogue multiplies by the gain, rounds, clamps, packs {I, Q} into 2 bytes -- with npol = 2 the first polarisation
//                waits in registers and both leave as one 4-byte {I0, Q0, I1, Q1} unit -- and passes through LDS, so that the rows
//                out[t][s][.][.] (2 F npol contiguous bytes) leave in whole 16-byte stores (2-byte stores when `out` is not 16-byte aligned:
//                the same bits).
// generic        every other F that clFFT takes, P > 16, and any handle under mi355_fengine_set_generic(h, 1): k_fe_woa forms z for a
//                bounded batch of (station, frame) pairs, an internal clFFT handle transforms it, k_fe_quant writes the frames.
//
// A frame's arithmetic does not depend on its place in a group, a call or a batch: any split of a stream into calls at frame boundaries
// and any legal alignment give the same bits within a route.
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "common.h"
#include "fft_core.hpp"

namespace {

using namespace fftc;
typedef float f2v __attribute__((ext_vector_type(2)));
typedef unsigned int u4v __attribute__((ext_vector_type(4)));

constexpr int kFePts = 4096;                    // points per frame group of the fused route
constexpr int kFePtrs = 64;                     // input pointers per launch (they travel as kernel arguments)
constexpr int kFeFusedTaps = 16;                // fused route: P <= 16
constexpr int kFeMaxTaps = 1024;
constexpr int kFeMaxInputs = 4096;              // S
constexpr long long kFeGenItems = 4ll << 20;    // generic route: values per batch (32 MiB each for z and X) unless one station's frame is larger
constexpr long long kFeMaxCall = 1ll << 40;     // bytes read per input and call
constexpr long long kFeHostBytes = 64ll << 20;  // host path: input bytes per staged piece unless one frame needs more

struct FeArgs {
    const f2v *in[kFePtrs];     // the launch's inputs, station-major; each at the first item of the call's first frame
    const float *taps;          // P N
    const float *gain;          // [r][N], the launch's first input first
    const c32 *tw;              // exp(-2 pi i k / N)
    unsigned long long *clips;  // the launch's first input first
    unsigned char *out;         // the call's first frame
    long long nframes;
    int P, S, s0;               // taps per channel; stations of a frame; the launch's first station
    int gpw, nchunks;           // frame groups per workgroup; workgroups per station
    int oxor, aligned;          // N / 2 with shift; `out` is 16-byte aligned
};

// one component: the int8 as the low byte; *clip counts a saturated or NaN component
__device__ __forceinline__ unsigned fe_q1(float v, unsigned &clip)
{
    const float r = __builtin_rintf(v);  // v_rndne_f32: half to even
    const bool sat = !(__builtin_fabsf(r) <= 127.f);  // NaN included
    clip += sat ? 1u : 0u;
    const float c = __builtin_fminf(__builtin_fmaxf(r, -127.f), 127.f);
    const int q = (v != v) ? 0 : (int)c;
    return (unsigned)q & 0xffu;
}

__device__ __forceinline__ unsigned fe_quant(c32 x, float g, bool count, unsigned &clip)
{
    unsigned c = 0;
    const unsigned pk = fe_q1(g * x.x, c) | (fe_q1(g * x.y, c) << 8);
    clip += count ? c : 0u;
    return pk;
}

template <int N, int NPOL>
__global__ __launch_bounds__(256, 2) void k_fengine(const FeArgs a)
{
    using G = Geo<N>;
    using PL = Plan<N>;
    static_assert(G::TH == 256 && G::PTS == kFePts, "geometry");
    constexpr int TH = 256, FG = G::F, NP = PL::NP, R0 = PL::radix(0), B0 = N / R0, RL = PL::radix(NP - 1), BL = N / RL;
    // N <= 64: consecutive elements per lane, redistributed through a padded LDS image -- as in k_fft and k_pspec
    constexpr bool SMALL = N <= 64;
    constexpr int PAD = B0 > 1 ? B0 : 1;
    constexpr int LDS_SLOTS = SMALL ? kFePts + FG * PAD : kFePts;
    __shared__ c32 lds[LDS_SLOTS];
    // the group's packed frames, [frame slot][f'][pol]{I, Q}: the image of FG output rows
    __shared__ __attribute__((aligned(16))) unsigned short stage[kFePts * NPOL];
    const int tid0 = threadIdx.x;
    const int sl = (int)blockIdx.x / a.nchunks, ch = (int)blockIdx.x - sl * a.nchunks;
    const long long kfirst = (long long)ch * a.gpw * FG;
    const long long kend = kfirst + (long long)a.gpw * FG < a.nframes ? kfirst + (long long)a.gpw * FG : a.nframes;
    const int nsteps = (int)((kend - kfirst + FG - 1) / FG) * NPOL;  // (group, polarisation) pairs, polarisation fastest
    const f2v *in0 = a.in[sl * NPOL], *in1 = a.in[sl * NPOL + (NPOL - 1)];
    const float *gain0 = a.gain + (long long)sl * NPOL * N;

    TwRegs<N> tw;
    load_twiddles<N, false, G>(tw, tid0, a.tw);

    // the taps of arm p at this thread's 16 points (N <= 64: one tap, every point of the thread has the same place in its frame)
    auto tapsof = [&](float (&h)[16], int p, int tid) {
        const float *t = a.taps + (long long)p * N;
        if constexpr (SMALL) {
            h[0] = t[tid % N];
        } else {
#pragma unroll
            for (int q = 0; q < 16 / R0; q++) {
                const int j = (tid + TH * q) % B0;
#pragma unroll
                for (int r = 0; r < R0; r++) h[q * R0 + r] = t[j + r * B0];
            }
        }
    };
    // Raw pass-0 inputs of a group: gp is the first item of the group's first frame (plus p N for arm p), `left` the frames the run still
    // has.  Branch free: a thread whose frame lies past the run reads the group's first frame instead (it exists, inside the call's
    // items) and keeps an exact zero.  P = 1 reads every item once: those loads stream (nt); with arms the frames are read again, through the caches.
    auto load = [&](c32 (&v)[16], const f2v *gp, int left, int tid, auto nt) {
        constexpr bool NT = decltype(nt)::value;
        if constexpr (SMALL) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const unsigned e = (unsigned)(tid + TH * k);
                const int fr = (int)(e / N), pos = (int)(e % N);
                const bool ok = fr < left;
                const f2v *q = gp + (long long)(ok ? fr : 0) * N + pos;
                const f2v x = NT ? __builtin_nontemporal_load(q) : *q;
                v[k] = ok ? mk(x.x, x.y) : mk(0.f, 0.f);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16 / R0; q++) {
                const int g = tid + TH * q, fr = g / B0;
                const bool ok = (FG == 1) || fr < left;
                const f2v *p = gp + (long long)(ok ? fr : 0) * N + (g % B0);
#pragma unroll
                for (int r = 0; r < R0; r++) {
                    const f2v x = NT ? __builtin_nontemporal_load(p + r * B0) : p[r * B0];
                    v[q * R0 + r] = ok ? mk(x.x, x.y) : mk(0.f, 0.f);
                }
            }
        }
    };
    auto gptr = [&](int it) { return ((NPOL == 2 && (it & 1)) ? in1 : in0) + (kfirst + (long long)(it / NPOL) * FG) * N; };
    auto leftof = [&](int it) {
        const long long l = kend - (kfirst + (long long)(it / NPOL) * FG);
        return (int)(l < FG ? l : FG);
    };
    float win[16];
    tapsof(win, 0, tid0);
    // z from the raw arm-0 items: arm 0 is a product, every further arm one fused multiply-add, p ascending
    auto arms = [&](c32 (&z)[16], const f2v *gp, int left, int tid) {
#pragma unroll
        for (int i = 0; i < 16; i++) z[i] = scale(z[i], win[SMALL ? 0 : i]);
        for (int p = 1; p < a.P; p++) {
            c32 x[16];
            float h[16];
            load(x, gp + (long long)p * N, left, tid, std::false_type());
            tapsof(h, p, tid);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float hv = h[SMALL ? 0 : i];
                z[i] = mk(fmaf(hv, x[i].x, z[i].x), fmaf(hv, x[i].y, z[i].y));
            }
        }
    };

    unsigned q0[16];  // npol = 2: the first polarisation's packed values wait here for the second
#pragma unroll
    for (int i = 0; i < 16; i++) q0[i] = 0;
    unsigned nclip0 = 0, nclip1 = 0;

    c32 cur[16];
    if (a.P == 1) load(cur, gptr(0), leftof(0), tid0, std::true_type());
    else load(cur, gptr(0), leftof(0), tid0, std::false_type());
    arms(cur, gptr(0), leftof(0), tid0);
    for (int it = 0; it < nsteps; it++) {
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int pol = NPOL == 2 ? (it & 1) : 0, left = leftof(it);
        c32 nxt[16];
        if (it + 1 < nsteps) {
            if (a.P == 1) load(nxt, gptr(it + 1), leftof(it + 1), tid, std::true_type());
            else load(nxt, gptr(it + 1), leftof(it + 1), tid, std::false_type());
        }
        float gn[16];  // the gains of this thread's 16 outputs
        {
            const float *gp = gain0 + pol * N;
#pragma unroll
            for (int q = 0; q < 16 / RL; q++) {
                const int j = (tid + TH * q) % BL;
#pragma unroll
                for (int s2 = 0; s2 < RL; s2++) gn[q * RL + s2] = gp[j + orev<RL>(s2) * BL];
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the transform
        c32 v[16];
        if constexpr (SMALL) {
            const int pos = tid % N, fr0 = tid / N;
#pragma unroll
            for (int k = 0; k < 16; k++) lds[(fr0 + k * (TH / N)) * (N + PAD) + pos] = cur[k];
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
            for (int i = 0; i < 16; i++) v[i] = cur[i];
        }
        transform_regs<N, -1, false, G>(v, tw, lds, tid);
        // v[q RL + s2] = X[fr][j + orev(s2) BL], g = tid + 256 q, fr = g / BL, j = g % BL
        unsigned nclip = 0;
#pragma unroll
        for (int q = 0; q < 16 / RL; q++) {
            const int g = tid + TH * q, fr = g / BL, j = g % BL;
            const bool ok = fr < left;
#pragma unroll
            for (int s2 = 0; s2 < RL; s2++) {
                const int i = q * RL + s2, fo = (j + orev<RL>(s2) * BL) ^ a.oxor;
                const unsigned pk = fe_quant(v[i], gn[i], ok, nclip);
                if constexpr (NPOL == 2) {
                    if (pol == 0) q0[i] = pk;
                    else ((unsigned *)stage)[fr * N + fo] = q0[i] | (pk << 16);
                } else {
                    stage[fr * N + fo] = (unsigned short)pk;
                }
            }
        }
        if (pol == 0) nclip0 += nclip;
        else nclip1 += nclip;
        __syncthreads();  // the packed rows are complete; the last pass' LDS reads are over
        if (pol == NPOL - 1) {
            // whole rows leave in 16-byte pieces; the next write to `stage` lies behind at least one barrier of the next transform
            constexpr int ROWB = 2 * N * NPOL, CPR = ROWB / 16, NCH = kFePts * 2 * NPOL / 16;
            const long long kg = kfirst + (long long)(it / NPOL) * FG;
#pragma unroll
            for (int i = 0; i < NCH / TH; i++) {
                const int c = tid + TH * i, fr = c / CPR, off = c % CPR;
                if (fr < left) {
                    unsigned char *dst = a.out + ((kg + fr) * (long long)a.S + (a.s0 + sl)) * ROWB + off * 16;
                    const u4v val = ((const u4v *)stage)[c];
                    if (a.aligned) {
                        __builtin_nontemporal_store(val, (u4v *)dst);
                    } else {
                        unsigned short *d2 = (unsigned short *)dst;
#pragma unroll
                        for (int w = 0; w < 4; w++) {
                            d2[2 * w] = (unsigned short)(val[w] & 0xffffu);
                            d2[2 * w + 1] = (unsigned short)(val[w] >> 16);
                        }
                    }
                }
            }
        }
        if (it + 1 < nsteps) {
#pragma unroll
            for (int i = 0; i < 16; i++) cur[i] = nxt[i];
            arms(cur, gptr(it + 1), leftof(it + 1), tid);
        }
    }

    // one integer atomic per wave and polarisation, and none where nothing clipped
#pragma unroll
    for (int p = 0; p < NPOL; p++) {
        unsigned c = p == 0 ? nclip0 : nclip1;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d, 64);
        if ((tid0 & 63) == 0 && c != 0) atomicAdd(a.clips + sl * NPOL + p, (unsigned long long)c);
    }
}

// ---- generic route ------------------------------------------------------------------------------------------------------------
struct FeGenArgs {
    const f2v *in[kFePtrs];  // the batch's inputs, each at the first item of the batch's first frame
    const float *taps;
    c32 *z;                  // [input][frame][n]
    int N, P, m;             // m: frames of the batch
    long long total;         // inputs m N
};

__global__ __launch_bounds__(256) void k_fe_woa(const FeGenArgs a)
{
    const long long per = (long long)a.m * a.N;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < a.total; idx += (long long)gridDim.x * 256) {
        const int ri = (int)(idx / per);
        const long long rem = idx - ri * per;  // t N + n
        const int n = (int)(rem % a.N);
        const f2v *x = a.in[ri] + rem;
        const f2v x0 = x[0];
        const float h0 = a.taps[n];
        float re = h0 * x0.x, im = h0 * x0.y;
        for (int p = 1; p < a.P; p++) {
            const f2v xp = x[(long long)p * a.N];
            const float h = a.taps[(long long)p * a.N + n];
            re = fmaf(h, xp.x, re);
            im = fmaf(h, xp.y, im);
        }
        a.z[idx] = mk(re, im);
    }
}

// X: [input of the batch][frame][f].  One thread per 2-byte output, in output order.
__global__ __launch_bounds__(256) void k_fe_quant(const c32 *__restrict__ X, const float *__restrict__ gain, unsigned long long *clips,
                                                  unsigned short *out, int N, int npol, int S, int s0, int Sb, int m, int half, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int pol = (int)(idx % npol);
        long long o = idx / npol;
        const int fo = (int)(o % N);
        o /= N;
        const int sl = (int)(o % Sb);
        const long long ti = o / Sb;
        const int rl = sl * npol + pol, f = fo + half < N ? fo + half : fo + half - N;  // f' = (f + N/2) mod N, N even
        const c32 x = X[((long long)rl * m + ti) * N + f];
        unsigned c = 0;
        const unsigned pk = fe_quant(x, gain[(long long)rl * N + f], true, c);
        out[((ti * S + s0 + sl) * N + fo) * npol + pol] = (unsigned short)pk;
        if (c) atomicAdd(clips + rl, (unsigned long long)c);
    }
}

bool fe_fused_size(int N, int P) { return N >= 16 && N <= 4096 && (N & (N - 1)) == 0 && P <= kFeFusedTaps; }

// what can be told without a device
int fe_check(int S, int npol, int N, int P, int shift)
{
    MI355_REQUIRE(npol == 1 || npol == 2, "npol must be 1 or 2");
    MI355_REQUIRE(S >= 1 && S <= kFeMaxInputs, "num_inputs must be 1 .. 4096");
    MI355_REQUIRE(N >= 2, "num_channels must be >= 2");
    MI355_REQUIRE(P >= 1 && P <= kFeMaxTaps, "taps_per_channel must be 1 .. 1024");
    MI355_REQUIRE(shift == 0 || shift == 1, "shift must be 0 or 1");
    MI355_REQUIRE(!shift || N % 2 == 0, "shift needs an even num_channels");
    char why[160];
    if (mi355_fft_plan_text(N, why, (int)sizeof why) != MI355_OK) {
        mi355_set_error("clFEngine: num_channels %d %s", N, why);  // clFFT's own words
        return MI355_ERR_UNSUPPORTED;
    }
    if ((long long)S * npol * N > (1ll << 28) || (long long)P * N > (1ll << 28)) {
        mi355_set_error("clFEngine: %d inputs of %d channels with %d taps each: a gain or tap table above 1 GiB", S * npol, N, P);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

}  // namespace

struct mi355_fengine {
    mi355_ctx *ctx = nullptr;
    int S = 0, npol = 1, R = 0, N = 0, P = 1, shift = 0;
    long long frame_bytes = 0;
    bool fused_ok = false, generic = false;
    std::vector<float> gains;             // the caller's layout, [r][N]
    mi355_tables gtab;                    // gains [r][N] on the device
    float *d_taps = nullptr;
    void *d_tw = nullptr;                 // fused route: exp(-2 pi i k / N)
    unsigned long long *d_clips = nullptr;
    mi355_fft *fft = nullptr;             // generic route, made when first needed
    // generic route: one workspace per handle; calls on different streams are ordered on it
    DevWorkspace ws;
    DevBuf d_in, d_out;  // host path staging
    std::string route;
    std::mutex lock;
};

namespace {

bool fe_is_fused(const mi355_fengine *h) { return h->fused_ok && !h->generic; }

void fe_gen_batch(const mi355_fengine *h, int *Sb, long long *nb)
{
    const long long per = (long long)h->npol * h->N;  // values per (station, frame)
    long long sb = kFePtrs / h->npol;
    if (sb > h->S) sb = h->S;
    if (sb * per > kFeGenItems) sb = kFeGenItems / per < 1 ? 1 : kFeGenItems / per;
    long long n = kFeGenItems / (sb * per);
    *Sb = (int)sb;
    *nb = n < 1 ? 1 : n;
}

void fe_name_route(mi355_fengine *h)
{
    char buf[160];
    if (fe_is_fused(h)) snprintf(buf, sizeof buf, "fused pow2 F=%d P=%d npol=%d group=%d", h->N, h->P, h->npol, kFePts / h->N);
    else {
        int Sb;
        long long nb;
        fe_gen_batch(h, &Sb, &nb);
        snprintf(buf, sizeof buf, "generic F=%d P=%d npol=%d batch=%dx%lld", h->N, h->P, h->npol, Sb, nb);
    }
    h->route = buf;
}

// a new version from h->gains; caller holds the lock (or is create) and has set the device
int fe_upload(mi355_fengine *h)
{
    return h->gtab.publish(h->ctx, h->gains.data(), h->gains.size() * sizeof(float), "mi355_fengine: gain");
}

#define FE_SIZES(X) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

int fe_launch_fused(mi355_fengine *h, long long n, const void *const *in, void *out, hipStream_t st)
{
    const int N = h->N, FG = kFePts / N;
    const long long cus = mi355_cus(h->ctx);
    const long long ngroups = (n + FG - 1) / FG;
    FeArgs a = {};
    a.taps = h->d_taps;
    a.tw = (const c32 *)h->d_tw;
    a.out = (unsigned char *)out;
    a.nframes = n;
    a.P = h->P;
    a.S = h->S;
    a.oxor = h->shift ? N / 2 : 0;
    a.aligned = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const int per = kFePtrs / h->npol;  // stations per launch
    for (int s0 = 0; s0 < h->S; s0 += per) {
        const int ns = h->S - s0 < per ? h->S - s0 : per;
        // about four workgroups per CU over the launch (two rounds of the two a CU holds), whole groups each: the longer a run, the
        // better the per-workgroup tables and the first, unhidden load are amortised
        long long want = (4 * cus + ns - 1) / ns;
        if (want > ngroups) want = ngroups;
        const long long gpw = (ngroups + want - 1) / want;
        const long long nchunks = (ngroups + gpw - 1) / gpw;
        if (gpw > (1ll << 30) / FG || nchunks * ns > (1ll << 30)) {
            mi355_set_error("clFEngine: %lld frames in one call", n);
            return MI355_ERR_UNSUPPORTED;
        }
        for (int i = 0; i < ns * h->npol; i++) a.in[i] = (const f2v *)in[s0 * h->npol + i];
        a.gain = (const float *)h->gtab.current() + (long long)s0 * h->npol * N;
        a.clips = h->d_clips + (long long)s0 * h->npol;
        a.s0 = s0;
        a.gpw = (int)gpw;
        a.nchunks = (int)nchunks;
        const dim3 grid((unsigned)(nchunks * ns));
#define X(NN)                                                                                        \
    if (N == NN) {                                                                                   \
        if (h->npol == 2) hipLaunchKernelGGL((k_fengine<NN, 2>), grid, dim3(256), 0, st, a);         \
        else hipLaunchKernelGGL((k_fengine<NN, 1>), grid, dim3(256), 0, st, a);                      \
    }
        FE_SIZES(X)
#undef X
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

int fe_launch_generic(mi355_fengine *h, long long n, const void *const *in, void *out, hipStream_t st)
{
    if (!h->fft) {
        const int rc = mi355_fft_create(h->ctx, h->N, MI355_FFT_FORWARD, nullptr, 0, MI355_DTYPE_COMPLEX, 1, 0, &h->fft);
        if (rc) return rc;
    }
    const int N = h->N, npol = h->npol;
    int Sb;
    long long nb;
    fe_gen_batch(h, &Sb, &nb);
    if (nb > n) nb = n;
    const size_t half = (size_t)Sb * npol * nb * N * 8;
    int rc = h->ws.acquire(2 * half, st);
    if (rc) return rc;
    c32 *d_z = (c32 *)h->ws.get(), *d_x = (c32 *)((char *)h->ws.get() + half);
    FeGenArgs g = {};
    g.taps = h->d_taps;
    g.z = d_z;
    g.N = N;
    g.P = h->P;
    for (long long t0 = 0; t0 < n; t0 += nb) {
        const long long m = n - t0 < nb ? n - t0 : nb;
        for (int s0 = 0; s0 < h->S; s0 += Sb) {
            const int ns = h->S - s0 < Sb ? h->S - s0 : Sb, nr = ns * npol;
            for (int i = 0; i < nr; i++) g.in[i] = (const f2v *)in[s0 * npol + i] + t0 * N;
            g.m = (int)m;
            g.total = (long long)nr * m * N;
            hipLaunchKernelGGL(k_fe_woa, dim3(mi355_grid_256(h->ctx, g.total, 32)), dim3(256), 0, st, g);
            rc = mi355_fft_work_dev(h->fft, (int)(nr * m), d_z, d_x, (void *)st);
            if (rc) return rc;
            hipLaunchKernelGGL(k_fe_quant, dim3(mi355_grid_256(h->ctx, g.total, 32)), dim3(256), 0, st, (const c32 *)d_x,
                               (const float *)h->gtab.current() + (long long)s0 * npol * N, h->d_clips + (long long)s0 * npol,
                               (unsigned short *)((char *)out + t0 * h->frame_bytes), N, npol, h->S, s0, ns, (int)m, h->shift ? N / 2 : 0, g.total);
        }
    }
    MI355_HIP(hipGetLastError());
    return h->ws.release(st);
}

// caller holds h->lock and has set the device
int fe_launch(mi355_fengine *h, long long n, const void *const *in, void *out, hipStream_t st)
{
    const int rc = fe_is_fused(h) ? fe_launch_fused(h, n, in, out, st) : fe_launch_generic(h, n, in, out, st);
    return rc ? rc : h->gtab.used(st);  // this version may be released behind this launch
}

int fe_args(const mi355_fengine *h, long long n, const void *const *in, const void *out)
{
    MI355_REQUIRE(n >= 0, "nframes is negative");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 1u) == 0, "out must be 2-byte aligned");
    const long long in_bytes = 8ll * h->N * (h->P - 1);
    if (n > (kFeMaxCall - in_bytes) / (8ll * h->N) || n > kFeMaxCall / h->frame_bytes) {
        mi355_set_error("clFEngine: %lld frames of %d channels in one call (the limit is 2^40 bytes per buffer)", n, h->N);
        return MI355_ERR_UNSUPPORTED;
    }
    const uintptr_t b = reinterpret_cast<uintptr_t>(out), blen = (uintptr_t)(n * h->frame_bytes), alen = (uintptr_t)(in_bytes + n * 8ll * h->N);
    for (int r = 0; r < h->R; r++) {
        MI355_REQUIRE(in[r] != nullptr, "NULL input");
        const uintptr_t a = reinterpret_cast<uintptr_t>(in[r]);
        MI355_REQUIRE((a & 7u) == 0, "every input must be 8-byte aligned");
        MI355_REQUIRE(!(a < b + blen && b < a + alen), "clFEngine does not work in place: an input overlaps out");
    }
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_fengine_plan(int num_inputs, int npol, int num_channels, int taps_per_channel, int shift, long long nframes,
                                  long long *frame_bytes, long long *history_items, long long *items_per_input)
{
    if (frame_bytes) *frame_bytes = 0;
    if (history_items) *history_items = 0;
    if (items_per_input) *items_per_input = 0;
    const int rc = fe_check(num_inputs, npol, num_channels, taps_per_channel, shift);
    if (rc) return rc;
    MI355_REQUIRE(nframes >= 0, "nframes is negative");
    const long long hist = (long long)(taps_per_channel - 1) * num_channels;
    if (nframes > ((1ll << 62) - hist) / num_channels) {
        mi355_set_error("clFEngine: %lld frames of %d channels: the item count passes 2^62", nframes, num_channels);
        return MI355_ERR_UNSUPPORTED;
    }
    if (frame_bytes) *frame_bytes = 2ll * num_inputs * num_channels * npol;
    if (history_items) *history_items = hist;
    if (items_per_input) *items_per_input = nframes == 0 ? 0 : nframes * num_channels + hist;
    return MI355_OK;
}

extern "C" int mi355_fengine_create(mi355_ctx *ctx, int num_inputs, int npol, int num_channels, int taps_per_channel, const float *taps, int shift,
                                    const float *gains, mi355_fengine **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    int rc = fe_check(num_inputs, npol, num_channels, taps_per_channel, shift);
    if (rc) return rc;
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_fengine *h = new (std::nothrow) mi355_fengine();
    if (!h) return MI355_ERR_NOMEM;
    const int N = num_channels, P = taps_per_channel;
    h->ctx = ctx; h->S = num_inputs; h->npol = npol; h->R = num_inputs * npol; h->N = N; h->P = P; h->shift = shift;
    h->frame_bytes = 2ll * num_inputs * N * npol;
    h->fused_ok = fe_fused_size(N, P);
    const size_t ng = (size_t)h->R * N, nt = (size_t)P * N;
    if (gains) h->gains.assign(gains, gains + ng);
    else h->gains.assign(ng, 1.0f);
    fe_name_route(h);
    auto fail = [&](int code) {
        mi355_fengine_destroy(h);
        return code;
    };
    if (hipSetDevice(ctx->device) != hipSuccess) {
        mi355_set_error("mi355_fengine_create: hipSetDevice failed");
        return fail(MI355_ERR_HIP);
    }
    {
        const std::vector<float> ones(taps ? 0 : nt, 1.0f);
        if (hipMalloc((void **)&h->d_taps, nt * sizeof(float)) != hipSuccess) return fail(MI355_ERR_NOMEM);
        if (mi355_upload(ctx, h->d_taps, taps ? taps : ones.data(), nt * sizeof(float)) != hipSuccess) return fail(MI355_ERR_HIP);
    }
    if (hipMalloc((void **)&h->d_clips, (size_t)h->R * 8) != hipSuccess) return fail(MI355_ERR_NOMEM);
    if (mi355_fill(ctx, h->d_clips, 0, (size_t)h->R * 8) != hipSuccess) return fail(MI355_ERR_HIP);
    if ((rc = fe_upload(h))) return fail(rc);
    if (h->fused_ok) {
        std::vector<float> tw((size_t)2 * N);
        for (int k = 0; k < N; k++) {
            const double a = -2.0 * M_PI * (double)k / (double)N;
            tw[2 * k] = (float)cos(a);
            tw[2 * k + 1] = (float)sin(a);
        }
        if (hipMalloc(&h->d_tw, tw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_NOMEM);
        if (mi355_upload(ctx, h->d_tw, tw.data(), tw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_HIP);
    }
    mi355_log(ctx, MI355_LOG_INFO, "clFEngine: %d stations, %d pol, %d channels, %d taps per channel, shift %d: %s", h->S, npol, N, P, shift,
              h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_fengine_destroy(mi355_fengine *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->gtab.release();
    (void)h->ws.wait();
    if (h->fft) (void)mi355_fft_destroy(h->fft);
    for (void *p : {(void *)h->d_taps, h->d_tw, (void *)h->d_clips})
        if (p) (void)hipFree(p);
    h->ws.destroy();
    for (DevBuf *b : {&h->d_in, &h->d_out}) b->release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_fengine_set_gains(mi355_fengine *h, const float *gains)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(gains != nullptr, "gains is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const std::vector<float> old = h->gains;
    h->gains.assign(gains, gains + old.size());
    const int rc = fe_upload(h);
    if (rc) h->gains = old;  // the version in use is still the old one
    return rc;
}

extern "C" int mi355_fengine_set_input_gain(mi355_fengine *h, int input, const float *gain)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(gain != nullptr, "gain is NULL");
    MI355_REQUIRE(input >= 0 && input < h->R, "input out of range");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const std::vector<float> old = h->gains;
    memcpy(h->gains.data() + (size_t)input * h->N, gain, sizeof(float) * (size_t)h->N);
    const int rc = fe_upload(h);
    if (rc) h->gains = old;
    return rc;
}

extern "C" int mi355_fengine_get_gains(const mi355_fengine *h, float *out, long long cap_floats)
{
    MI355_REQUIRE(h && out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_fengine *>(h)->lock);
    MI355_REQUIRE(cap_floats >= (long long)h->gains.size(), "out too small");
    memcpy(out, h->gains.data(), h->gains.size() * sizeof(float));
    return MI355_OK;
}

extern "C" int mi355_fengine_get_clips(mi355_fengine *h, unsigned long long *out, int reset)
{
    MI355_REQUIRE(h && out, "NULL argument");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    MI355_HIP(hipDeviceSynchronize());  // every call of the handle enqueued so far, on whatever stream, has counted
    MI355_HIP(hipMemcpy(out, h->d_clips, (size_t)h->R * 8, hipMemcpyDeviceToHost));
    if (reset) MI355_HIP(hipMemset(h->d_clips, 0, (size_t)h->R * 8));
    return MI355_OK;
}

extern "C" int mi355_fengine_set_generic(mi355_fengine *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    fe_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_fengine_route(const mi355_fengine *h) { return h ? h->route.c_str() : ""; }
extern "C" long long mi355_fengine_frame_bytes(const mi355_fengine *h) { return h ? h->frame_bytes : MI355_ERR_INVALID_ARG; }
extern "C" long long mi355_fengine_history_items(const mi355_fengine *h) { return h ? (long long)(h->P - 1) * h->N : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_fengine_work_dev(mi355_fengine *h, long long nframes, const void *const *in_with_history, void *out, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = fe_args(h, nframes, in_with_history, out);
    if (rc || nframes == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return fe_launch(h, nframes, in_with_history, out, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_fengine_work(mi355_fengine *h, long long nframes, const void *const *in_with_history, void *out)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = fe_args(h, nframes, in_with_history, out);
    if (rc || nframes == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole frames; a piece re-sends the (P - 1) N items of history it shares with the piece before
    const long long hist = (long long)(h->P - 1) * h->N;
    const long long per_frame = 8ll * h->N * h->R > h->frame_bytes ? 8ll * h->N * h->R : h->frame_bytes;
    const long long piece = mi355_piece_units(kFeHostBytes / per_frame, nframes);
    const size_t stride = (size_t)(piece * h->N + hist) * 8;  // bytes per input in the staging buffer
    if ((rc = h->d_in.reserve(stride * h->R))) return rc;
    if ((rc = h->d_out.reserve((size_t)(piece * h->frame_bytes)))) return rc;
    std::vector<const void *> ptrs((size_t)h->R);
    for (int r = 0; r < h->R; r++) ptrs[r] = (const char *)h->d_in.get() + stride * r;
    return mi355_pageable_run(h->ctx, nframes, piece, [&](long long t0, long long m, hipStream_t st) -> int {
        for (int r = 0; r < h->R; r++)
            MI355_HIP(hipMemcpyAsync((char *)h->d_in.get() + stride * r, (const char *)in_with_history[r] + t0 * h->N * 8, (size_t)(m * h->N + hist) * 8,
                                     hipMemcpyHostToDevice, st));
        const int lrc = fe_launch(h, m, ptrs.data(), h->d_out.get(), st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + t0 * h->frame_bytes, h->d_out.get(), (size_t)(m * h->frame_bytes), hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
}
