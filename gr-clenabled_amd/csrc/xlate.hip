// clFreqXlatingFIRFilter: tune + FIR + decimate for C channels of one wideband stream as gfx950 HIP kernels.  The contract is GNU Radio's
// freq_xlating_fir_filter_ccf / ccc, restated in include/mi355_clenabled.h; the reference module has no such block.
//
//     y_c[m] = r_c(m) sum_k b_c[k] x[m D - k],   b_c[k] = h[k] exp(+j 2 pi frac(k f_c / fs)),   r_c(m) = exp(-j 2 pi P_c(m) / 2^64)
//
// with P_c(m) = P_c(0) + inc_c m in unsigned 64-bit arithmetic: the phase of an output is a pure function of its index, so any split of
// a stream into calls gives the same bits and nothing drifts.  The device table holds every channel's band-pass taps reversed and zero
// padded to KP = a multiple of eight, so an output is a dot product with the ascending window in[m D .. m D + K) of the history-prefixed
// buffer.
//
// k_xlate     the fused route.  A workgroup keeps the C tap sets in LDS and walks tiles of tile_out outputs: the tile's span
//             (tile_out - 1) D + K samples is staged ONCE, as sample pairs with 16-byte loads (the slot padding of k_fir_dec2 in filter.hip:
//             xl_pad_shift is a private copy of dec2_pad_shift), and every wave then takes (64 outputs, CB channels) units of the tile:
//             four 16-byte sample reads serve CB channels' eight taps each, the taps are wave-uniform broadcast reads.  One fmaf chain
//             per component over k ascending, then one complex multiply by the phasor (one double sincospi per output and channel),
//             then an 8-byte store into the channel's own buffer.
//             A window starts on the second sample of a pair when D is odd and the output index is, or when `in` is only 8-byte
//             aligned (the tile is then staged from the 16-byte boundary below and every window moves by one sample); the outputs are
//             dealt so that a wave's windows all start alike, and such a wave reads five units per step and uses them shifted by one
//             sample.  The arithmetic is the same in both forms, so every legal alignment gives the same bits.
//             Items before in[0] and past in[(n - 1) D + K) are never loaded (the pair that straddles either end is loaded as single
//             items), and the last tap step masks the samples past the window, so no product touches a sample outside it.
// k_xl_rotate the generic route's second step: y[m] *= r(m) in place, after the channel's internal clComplexFilter handle (band-pass
//             taps, decimation D, the caller's use_time choice) has written y.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"

namespace {

typedef float2 c32;
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kXlThreads = 256;
constexpr int kXlMaxFusedC = 16, kXlMaxFusedK = 512, kXlMaxFusedD = 64;
constexpr int kXlMaxChannels = 4096;
constexpr int kXlLdsBytes = 160 << 10;
constexpr int kXlMetaBytes = kXlMaxFusedC * 3 * 8;  // phase, increment and output pointer of every channel, in LDS

struct XlArgs {
    c32 *out[kXlMaxFusedC];
    u64 phase[kXlMaxFusedC], inc[kXlMaxFusedC];
};

// pair p sits at 16-byte unit p + (p >> sh); see k_fir_dec2 (filter.hip): multiples of 8 need one unit of padding per 32, every other
// decimation is conflict free or nearly so without
__host__ __device__ inline int xl_unit(int p, int sh) { return p + (p >> sh); }
inline int xl_pad_shift(int decim) { return decim % 8 == 0 ? 5 : 31; }

// the phasor of absolute phase P and the final complex multiply; both routes use this one function
__device__ __forceinline__ c32 xl_rotate(float ax, float ay, u64 P)
{
    // P / 2^64 turns, taken as a signed fraction so that small negative angles keep their precision: 2 turns = P_signed / 2^63
    const double t2 = (double)(long long)P * 0x1p-63;
    double sn, cs;
    sincospi(t2, &sn, &cs);
    const float cr = (float)cs, ci = (float)(-sn);  // r = exp(-j 2 pi P / 2^64)
    return make_float2(fmaf(ax, cr, -(ay * ci)), fmaf(ax, ci, ay * cr));
}

template <int CB, bool ODD>
__global__ __launch_bounds__(kXlThreads) void k_xlate(const c32 *__restrict__ in, const XlArgs a, const float *__restrict__ taps, int C, int K,
                                                      int KP, int D, long long n_out, int tile_out, int sh, int aoff)
{
    extern __shared__ __attribute__((aligned(16))) v4f xl_lds[];
    u64 *const meta = (u64 *)xl_lds;                            // [3][kXlMaxFusedC]
    v4f *const tl = xl_lds + kXlMetaBytes / 16;                 // taps: C sets of 2 KP floats
    const int tap_units = C * (KP >> 1);
    v4f *const xl = tl + tap_units;                             // sample pairs
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < kXlMaxFusedC; i++)  // (constant indices: the argument block stays in scalar registers)
        if (tid == i) {
            meta[i] = a.phase[i];
            meta[kXlMaxFusedC + i] = a.inc[i];
            meta[2 * kXlMaxFusedC + i] = (u64)(uintptr_t)a.out[i];
        }
    for (int i = tid; i < tap_units; i += kXlThreads) tl[i] = ((const v4f *)taps)[i];
    const long long n_in = (n_out - 1) * D + K;  // the samples the outputs need: in[0 .. n_in)
    const long long ntiles = (n_out + tile_out - 1) / tile_out;
    const int wave = tid >> 6, lane = tid & 63;
    const int G = C / CB;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long o0 = tile * tile_out, left = n_out - o0;
        const int no = left < tile_out ? (int)left : tile_out;
        const long long b = o0 * D - aoff;  // item index of the first staged sample: even + the alignment offset, so in + b sits on 16 bytes
        const v4f *__restrict__ src = (const v4f *)(in + b);
        const int pairs = (((no - 1) * D + aoff) >> 1) + (KP >> 1) + 1;
        __syncthreads();  // the previous tile's reads are done; the first time: taps and meta are written
        for (int p0 = 0; p0 < pairs; p0 += 8 * kXlThreads) {
            v4f v[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int p = p0 + j * kXlThreads + tid;
                v[j] = (v4f){0.f, 0.f, 0.f, 0.f};
                if (p < pairs) {
                    const long long i0 = b + 2LL * p;
                    if (i0 >= 0 && i0 + 1 < n_in) v[j] = __builtin_nontemporal_load(src + p);
                    else {
                        if (i0 >= 0 && i0 < n_in) { const c32 s = in[i0]; v[j][0] = s.x; v[j][1] = s.y; }
                        if (i0 + 1 >= 0 && i0 + 1 < n_in) { const c32 s = in[i0 + 1]; v[j][2] = s.x; v[j][3] = s.y; }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int p = p0 + j * kXlThreads + tid;
                if (p < pairs) xl[xl_unit(p, sh)] = v[j];
            }
        }
        __syncthreads();
        // units of (64 outputs, CB channels); odd D: the even and the odd outputs of 128 are two units
        const int nu = ODD ? 2 * ((no + 127) >> 7) : (no + 63) >> 6;
        for (int u = wave; u < G * nu; u += kXlThreads / 64) {
            const int g = u / nu, r = u - g * nu;
            const int o = ODD ? (r >> 1) * 128 + 2 * lane + (r & 1) : r * 64 + lane;
            if (o >= no) continue;
            const int w = o * D + aoff, pb = w >> 1;
            const bool shifted = ODD ? (((r & 1) ^ aoff) != 0) : (aoff != 0);  // = w & 1, wave-uniform
            float ax[CB], ay[CB];
#pragma unroll
            for (int cb = 0; cb < CB; cb++) ax[cb] = ay[cb] = 0.f;
            const v4f *const tg = tl + (size_t)g * CB * (KP >> 1);
            for (int k = 0; k < KP; k += 8) {
                v4f sm[4];
                if (shifted) {
                    v4f un[5];
#pragma unroll
                    for (int j = 0; j < 5; j++) un[j] = xl[xl_unit(pb + (k >> 1) + j, sh)];
#pragma unroll
                    for (int j = 0; j < 4; j++) sm[j] = (v4f){un[j][2], un[j][3], un[j + 1][0], un[j + 1][1]};
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++) sm[j] = xl[xl_unit(pb + (k >> 1) + j, sh)];
                }
                if (k + 8 > K) {  // the last step: samples past the window are dropped, whatever they hold (uniform)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        if (k + 2 * j >= K) { sm[j][0] = 0.f; sm[j][1] = 0.f; }
                        if (k + 2 * j + 1 >= K) { sm[j][2] = 0.f; sm[j][3] = 0.f; }
                    }
                }
#pragma unroll
                for (int cb = 0; cb < CB; cb++) {
                    v4f t[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) t[j] = tg[cb * (KP >> 1) + (k >> 1) + j];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        ax[cb] = fmaf(t[j][0], sm[j][0], ax[cb]); ax[cb] = fmaf(-t[j][1], sm[j][1], ax[cb]);
                        ay[cb] = fmaf(t[j][0], sm[j][1], ay[cb]); ay[cb] = fmaf(t[j][1], sm[j][0], ay[cb]);
                        ax[cb] = fmaf(t[j][2], sm[j][2], ax[cb]); ax[cb] = fmaf(-t[j][3], sm[j][3], ax[cb]);
                        ay[cb] = fmaf(t[j][2], sm[j][3], ay[cb]); ay[cb] = fmaf(t[j][3], sm[j][2], ay[cb]);
                    }
                }
            }
            const u64 m = (u64)(o0 + o);
#pragma unroll
            for (int cb = 0; cb < CB; cb++) {
                const int c = g * CB + cb;
                const c32 y = xl_rotate(ax[cb], ay[cb], meta[c] + meta[kXlMaxFusedC + c] * m);
                c32 *const dst = (c32 *)(uintptr_t)meta[2 * kXlMaxFusedC + c];
                __builtin_nontemporal_store((v2f){y.x, y.y}, (v2f *)(dst + o0 + o));
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_xl_rotate(c32 *__restrict__ y, long long n, u64 phase, u64 inc)
{
    for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < n; m += (long long)gridDim.x * 256) {
        const c32 s = y[m];
        y[m] = xl_rotate(s.x, s.y, phase + inc * (u64)m);
    }
}

int xl_check(int D, int K)
{
    MI355_REQUIRE(D >= 1, "decimation must be >= 1");
    MI355_REQUIRE(K >= 1, "at least one tap");
    return MI355_OK;
}

constexpr long long kXlMaxCall = 1ll << 44;

}  // namespace

struct mi355_xlate {
    mi355_ctx *ctx = nullptr;
    int D = 1, K = 0, KP = 0, C = 0, complex_taps = 0, use_time = 0;
    double fs = 1.0;
    std::vector<double> freq;               // C
    std::vector<float> taps_host;           // K floats, or 2 K for a complex prototype
    std::vector<std::vector<float>> bp;     // per channel: the band-pass taps b_c as 2 K floats, k ascending
    std::vector<u64> phase, inc;            // host state: P_c of the next output, and its increment per output
    bool fused = false, generic = false;    // the shape has a fused route; the generic route is forced
    int tile_out = 0, sh = 31, lds_bytes = 0, cb = 1, wg_per_cu = 1;
    mi355_tables tab;                       // [C][2 KP] reversed, zero padded (fused shapes only)
    std::vector<mi355_filter *> filt;       // generic route: one internal clComplexFilter handle per channel (made when first needed)
    HostPipe pipe;
    std::string route;
    std::mutex lock;
};

namespace {

// the fused route of a shape: a function of (D, K, C) alone
void xl_choose(mi355_xlate *h)
{
    h->fused = false;
    h->KP = (h->K + 7) / 8 * 8;
    if (h->D < 2 || h->D > kXlMaxFusedD || h->K > kXlMaxFusedK || h->C > kXlMaxFusedC) return;
    const int span_max = h->K <= 128 ? 3072 : 4096;  // samples per tile, as k_fir_dec2; at least 128 outputs whatever D
    int tile = span_max > h->KP ? (span_max - h->KP) / h->D + 1 : 1;
    if (tile > 2048) tile = 2048;
    tile = tile < 128 ? 128 : tile / 128 * 128;
    const int sh = xl_pad_shift(h->D);
    const int pairs = (((tile - 1) * h->D + 1) >> 1) + (h->KP >> 1) + 1;
    const long long bytes = (long long)kXlMetaBytes + ((long long)h->C * (h->KP >> 1) + xl_unit(pairs, sh) + 2) * 16;
    if (bytes > kXlLdsBytes) return;
    h->fused = true;
    h->tile_out = tile; h->sh = sh; h->lds_bytes = (int)bytes;
    h->cb = h->C % 4 == 0 ? 4 : (h->C % 2 == 0 ? 2 : 1);
    const int k = kXlLdsBytes / h->lds_bytes;
    h->wg_per_cu = k > 8 ? 8 : k;
}

void xl_name_route(mi355_xlate *h)
{
    char buf[160];
    if (h->fused && !h->generic) snprintf(buf, sizeof buf, "fused D=%d K=%d C=%d tile_out=%d", h->D, h->K, h->C, h->tile_out);
    else snprintf(buf, sizeof buf, "generic D=%d K=%d C=%d", h->D, h->K, h->C);
    h->route = buf;
}

// round(frac(f D / fs) 2^64) mod 2^64, evaluated on the signed fraction nearest zero: a small negative frequency keeps its precision
// and -f gives exactly the negated increment
u64 xl_inc(double f, int D, double fs)
{
    double t = f * (double)D / fs;
    t -= std::nearbyint(t);  // [-0.5, 0.5]
    const double v = std::nearbyint(std::ldexp(t, 64));
    return v >= 0x1p63 ? 1ull << 63 : (u64)(long long)v;
}

void xl_bandpass(mi355_xlate *h, int c)
{
    const double ratio = h->freq[c] / h->fs;
    std::vector<float> &b = h->bp[c];
    b.resize((size_t)2 * h->K);
    for (int k = 0; k < h->K; k++) {
        double t = (double)k * ratio;
        t -= std::floor(t);
        const double ang = 2.0 * M_PI * t, cs = std::cos(ang), sn = std::sin(ang);
        const double hr = h->complex_taps ? h->taps_host[2 * (size_t)k] : h->taps_host[k], hi = h->complex_taps ? h->taps_host[2 * (size_t)k + 1] : 0.0;
        b[2 * (size_t)k] = (float)(hr * cs - hi * sn);
        b[2 * (size_t)k + 1] = (float)(hr * sn + hi * cs);
    }
}

// the device table of the fused route from bp[]; caller holds the lock (or is create) and has set the device
int xl_upload(mi355_xlate *h)
{
    if (!h->fused) { h->tab.drop(); return MI355_OK; }
    const size_t per = (size_t)2 * h->KP;
    std::vector<float> tab(per * h->C, 0.f);
    for (int c = 0; c < h->C; c++)
        for (int i = 0; i < h->K; i++) {
            tab[c * per + 2 * (size_t)i] = h->bp[c][2 * (size_t)(h->K - 1 - i)];
            tab[c * per + 2 * (size_t)i + 1] = h->bp[c][2 * (size_t)(h->K - 1 - i) + 1];
        }
    return h->tab.publish(h->ctx, tab.data(), tab.size() * sizeof(float), "mi355_xlate: table");
}

void xl_drop_filters(mi355_xlate *h)
{
    for (mi355_filter *f : h->filt) mi355_filter_destroy(f);
    h->filt.clear();
}

// the generic route's internal handles; caller holds the lock (or is create)
int xl_make_filters(mi355_xlate *h)
{
    if (!h->filt.empty()) return MI355_OK;
    for (int c = 0; c < h->C; c++) {
        mi355_filter *f = nullptr;
        const int rc = mi355_filter_create(h->ctx, h->D, h->bp[c].data(), h->K, 1, h->use_time, &f);
        if (rc) { xl_drop_filters(h); return rc; }
        h->filt.push_back(f);
    }
    return MI355_OK;
}

// taps (and with them K) of a handle: band-pass sets, route, table, filters.  On failure the handle keeps what it had.
int xl_set_taps(mi355_xlate *h, const void *taps, int K)
{
    MI355_REQUIRE(taps != nullptr, "taps is NULL");
    int rc = xl_check(h->D, K);
    if (rc) return rc;
    const int E = h->complex_taps ? 2 : 1;
    const float *t = (const float *)taps;
    const std::vector<float> old_taps = h->taps_host;
    const int old_K = h->K;
    h->taps_host.assign(t, t + (size_t)K * E);
    h->K = K;
    for (int c = 0; c < h->C; c++) xl_bandpass(h, c);
    xl_choose(h);
    rc = xl_upload(h);
    if (rc == MI355_OK) {
        if (!h->fused || h->generic) {
            if (old_K == K && !h->filt.empty()) {
                for (int c = 0; c < h->C && rc == MI355_OK; c++) rc = mi355_filter_set_taps(h->filt[c], h->bp[c].data(), K);
            } else {
                xl_drop_filters(h);
                rc = xl_make_filters(h);
            }
        } else {
            xl_drop_filters(h);
        }
    }
    if (rc) {  // back to the taps before (no device work can fail on the way: the old table is still the current one unless upload succeeded)
        if (old_K > 0) {
            h->taps_host = old_taps;
            h->K = old_K;
            for (int c = 0; c < h->C; c++) xl_bandpass(h, c);
            xl_choose(h);
            (void)xl_upload(h);
            xl_drop_filters(h);
            if (!h->fused || h->generic) (void)xl_make_filters(h);
        }
        return rc;
    }
    xl_name_route(h);
    mi355_log(h->ctx, MI355_LOG_INFO, "clFreqXlatingFIRFilter: decimation %d, %d %s taps, %d channel%s: %s%s", h->D, K, h->complex_taps ? "complex" : "real",
              h->C, h->C == 1 ? "" : "s", h->route.c_str(), h->fused && !h->generic ? " (k_xlate)" : " (clComplexFilter + k_xl_rotate per channel)");
    return MI355_OK;
}

// caller holds the lock and has set the device; `phase`: P_c of output 0 of this launch
int xl_launch(mi355_xlate *h, long long n, const void *in, void *const *outs, const u64 *phase, hipStream_t st)
{
    const int cus = mi355_cus(h->ctx);
    if (h->fused && !h->generic) {
        XlArgs a = {};
        for (int c = 0; c < h->C; c++) { a.out[c] = (c32 *)outs[c]; a.phase[c] = phase[c]; a.inc[c] = h->inc[c]; }
        const long long tiles = (n + h->tile_out - 1) / h->tile_out, cap = (long long)cus * h->wg_per_cu;
        const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
        const int aoff = (int)((reinterpret_cast<uintptr_t>(in) >> 3) & 1u);
#define XL_LAUNCH(CB, OD)                                                                                                              \
    do {                                                                                                                               \
        MI355_HIP(hipFuncSetAttribute((const void *)k_xlate<CB, OD>, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes));        \
        hipLaunchKernelGGL((k_xlate<CB, OD>), grid, dim3(kXlThreads), (size_t)h->lds_bytes, st, (const c32 *)in, a, (const float *)h->tab.current(), h->C, h->K, \
                           h->KP, h->D, n, h->tile_out, h->sh, aoff);                                                                  \
    } while (0)
#define XL_CASE(CB) do { if (h->D % 2) XL_LAUNCH(CB, true); else XL_LAUNCH(CB, false); } while (0)
        if (h->cb == 4) XL_CASE(4);
        else if (h->cb == 2) XL_CASE(2);
        else XL_CASE(1);
#undef XL_CASE
#undef XL_LAUNCH
        MI355_HIP(hipGetLastError());
        return MI355_OK;
    }
    if (h->filt.empty()) {
        mi355_set_error("clFreqXlatingFIRFilter: the generic route has no filter handles (the last set_taps failed)");
        return MI355_ERR_STATE;
    }
    const long long blocks = (n + 255) / 256, cap = (long long)cus * 16;
    for (int c = 0; c < h->C; c++) {
        const int rc = mi355_filter_work_dev(h->filt[c], (size_t)n, in, outs[c], (void *)st);
        if (rc) return rc;
        hipLaunchKernelGGL(k_xl_rotate, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, st, (c32 *)outs[c], n, phase[c], h->inc[c]);
        MI355_HIP(hipGetLastError());
    }
    return MI355_OK;
}

int xl_args(mi355_xlate *h, long long n, const void *in, void *const *outs)
{
    MI355_REQUIRE(n >= 0, "noutput is negative");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && outs, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 7u) == 0, "buffers must be 8-byte aligned");
    if (n > kXlMaxCall / h->D) {
        mi355_set_error("clFreqXlatingFIRFilter: %lld outputs at decimation %d in one call", n, h->D);
        return MI355_ERR_UNSUPPORTED;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), a_end = a + ((uintptr_t)n * h->D + h->K - 1) * 8;
    for (int c = 0; c < h->C; c++) {
        MI355_REQUIRE(outs[c] != nullptr, "NULL output buffer");
        const uintptr_t b = reinterpret_cast<uintptr_t>(outs[c]);
        MI355_REQUIRE((b & 7u) == 0, "buffers must be 8-byte aligned");
        MI355_REQUIRE(!(a < b + (uintptr_t)n * 8 && b < a_end), "clFreqXlatingFIRFilter does not work in place: in and an output overlap");
    }
    return MI355_OK;
}

bool xl_chan(const mi355_xlate *h, int c) { return h && c >= 0 && c < h->C; }

}  // namespace

extern "C" int mi355_xlate_plan(int decimation, int ntaps, long long noutput, long long *ninput_items, int *history)
{
    if (ninput_items) *ninput_items = 0;
    if (history) *history = 0;
    const int rc = xl_check(decimation, ntaps);
    if (rc) return rc;
    MI355_REQUIRE(noutput >= 0, "noutput is negative");
    if (noutput > (1ll << 62) / decimation) {
        mi355_set_error("clFreqXlatingFIRFilter: %lld outputs at decimation %d", noutput, decimation);
        return MI355_ERR_UNSUPPORTED;
    }
    if (ninput_items) *ninput_items = noutput == 0 ? 0 : noutput * decimation + ntaps - 1;
    if (history) *history = ntaps;
    return MI355_OK;
}

extern "C" int mi355_xlate_create(mi355_ctx *ctx, int decimation, const void *taps, int ntaps, int complex_taps, double samp_rate,
                                  const double *center_freqs, int nfreq, int use_time, mi355_xlate **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    int rc = xl_check(decimation, ntaps);
    if (rc) return rc;
    MI355_REQUIRE(taps != nullptr, "taps is NULL");
    MI355_REQUIRE(nfreq >= 1, "at least one centre frequency");
    MI355_REQUIRE(center_freqs != nullptr, "center_freqs is NULL");
    MI355_REQUIRE(std::isfinite(samp_rate) && samp_rate > 0.0, "the sample rate must be finite and > 0");
    for (int c = 0; c < nfreq; c++) MI355_REQUIRE(std::isfinite(center_freqs[c]), "a centre frequency is not finite");
    if (nfreq > kXlMaxChannels) {
        mi355_set_error("clFreqXlatingFIRFilter: %d channels, the limit is %d", nfreq, kXlMaxChannels);
        return MI355_ERR_UNSUPPORTED;
    }
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_xlate *h = new (std::nothrow) mi355_xlate();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->D = decimation; h->C = nfreq; h->complex_taps = complex_taps ? 1 : 0; h->use_time = use_time ? 1 : 0; h->fs = samp_rate;
    h->freq.assign(center_freqs, center_freqs + nfreq);
    h->bp.resize(nfreq);
    h->phase.assign(nfreq, 0ull);
    h->inc.resize(nfreq);
    for (int c = 0; c < nfreq; c++) h->inc[c] = xl_inc(h->freq[c], h->D, h->fs);
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_xlate_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = xl_set_taps(h, taps, ntaps);
        if (rc == MI355_OK) rc = h->pipe.init(ctx);
    }
    if (rc) { mi355_xlate_destroy(h); return rc; }
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_xlate_destroy(mi355_xlate *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    xl_drop_filters(h);
    h->tab.release();
    h->pipe.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_xlate_set_taps(mi355_xlate *h, const void *taps, int ntaps)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return xl_set_taps(h, taps, ntaps);  // every phase is kept
}

extern "C" int mi355_xlate_ntaps(const mi355_xlate *h) { return h ? h->K : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_xlate_num_channels(const mi355_xlate *h) { return h ? h->C : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_xlate_decimation(const mi355_xlate *h) { return h ? h->D : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_xlate_get_taps(const mi355_xlate *h, void *taps_out, int cap)
{
    MI355_REQUIRE(h && taps_out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_xlate *>(h)->lock);
    MI355_REQUIRE(cap >= h->K, "taps_out too small");
    memcpy(taps_out, h->taps_host.data(), h->taps_host.size() * sizeof(float));
    return h->K;
}

extern "C" int mi355_xlate_get_bandpass_taps(const mi355_xlate *h, int c, void *out, int cap)
{
    MI355_REQUIRE(h && out, "NULL argument");
    MI355_REQUIRE(xl_chan(h, c), "channel out of range");
    std::lock_guard<std::mutex> g(const_cast<mi355_xlate *>(h)->lock);
    MI355_REQUIRE(cap >= h->K, "out too small");
    memcpy(out, h->bp[c].data(), h->bp[c].size() * sizeof(float));
    return h->K;
}

extern "C" int mi355_xlate_set_center_freq(mi355_xlate *h, int c, double freq)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(xl_chan(h, c), "channel out of range");
    MI355_REQUIRE(std::isfinite(freq), "the centre frequency is not finite");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const double old = h->freq[c];
    h->freq[c] = freq;
    xl_bandpass(h, c);
    int rc = xl_upload(h);
    if (rc == MI355_OK && !h->filt.empty()) rc = mi355_filter_set_taps(h->filt[c], h->bp[c].data(), h->K);
    if (rc) {  // the table in use is still the old one
        h->freq[c] = old;
        xl_bandpass(h, c);
        return rc;
    }
    h->inc[c] = xl_inc(freq, h->D, h->fs);  // P_c stays: the phase is continuous across a retune
    return MI355_OK;
}

extern "C" int mi355_xlate_get_center_freq(const mi355_xlate *h, int c, double *freq)
{
    MI355_REQUIRE(h && freq, "NULL argument");
    MI355_REQUIRE(xl_chan(h, c), "channel out of range");
    std::lock_guard<std::mutex> g(const_cast<mi355_xlate *>(h)->lock);
    *freq = h->freq[c];
    return MI355_OK;
}

extern "C" int mi355_xlate_get_state(const mi355_xlate *h, int c, unsigned long long *phase, unsigned long long *inc)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(xl_chan(h, c), "channel out of range");
    std::lock_guard<std::mutex> g(const_cast<mi355_xlate *>(h)->lock);
    if (phase) *phase = h->phase[c];
    if (inc) *inc = h->inc[c];
    return MI355_OK;
}

extern "C" int mi355_xlate_set_phase(mi355_xlate *h, int c, unsigned long long phase)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(xl_chan(h, c), "channel out of range");
    std::lock_guard<std::mutex> g(h->lock);
    h->phase[c] = phase;
    return MI355_OK;
}

extern "C" int mi355_xlate_skip(mi355_xlate *h, long long noutputs)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(noutputs >= 0, "noutputs is negative");
    std::lock_guard<std::mutex> g(h->lock);
    for (int c = 0; c < h->C; c++) h->phase[c] += h->inc[c] * (u64)noutputs;
    return MI355_OK;
}

extern "C" int mi355_xlate_set_generic(mi355_xlate *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    if (on) {
        const int rc = xl_make_filters(h);
        if (rc) return rc;
    }
    h->generic = on != 0;
    xl_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_xlate_route(const mi355_xlate *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_xlate_work_dev(mi355_xlate *h, long long noutput, const void *in_with_history, void *const *outs, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = xl_args(h, noutput, in_with_history, outs);
    if (rc || noutput == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = mi355_pick_stream(h->ctx, stream);
    rc = xl_launch(h, noutput, in_with_history, outs, h->phase.data(), st);
    if (rc == MI355_OK && h->fused && !h->generic) rc = h->tab.used(st);  // this table may be released behind this launch
    if (rc) return rc;
    for (int c = 0; c < h->C; c++) h->phase[c] += h->inc[c] * (u64)noutput;  // the phase is a kernel argument: no device state
    return MI355_OK;
}

extern "C" int mi355_xlate_work(mi355_xlate *h, long long noutput, const void *in_with_history, void *const *outs)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = xl_args(h, noutput, in_with_history, outs);
    if (rc || noutput == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of outputs sized from the larger side, the input; each piece re-sends its K - 1 samples of history.  One staging slot: the
    // pieces run one after the other.
    const size_t hist = (size_t)h->K - 1;
    size_t piece = mi355_chunk_bytes((size_t)noutput * h->D * 8, h->ctx) / (8 * (size_t)h->D);
    if (piece < 1) piece = 1;
    if (piece > (size_t)noutput) piece = (size_t)noutput;
    const size_t in_cap = (piece * h->D + hist) * 8;
    rc = h->pipe.ensure(1, &in_cap, piece * 8 * h->C, 1);
    if (rc) return rc;
    const HostPipe::Plan plan{1, true, false};  // one slot, stream[0], never direct
    auto outputs = [&](size_t ci) { return HostPipe::part((size_t)noutput, piece, ci); };
    std::vector<u64> ph(h->C);
    std::vector<void *> d_outs(h->C);
    rc = h->pipe.run(
        ((size_t)noutput + piece - 1) / piece, plan,
        [&](size_t ci) {  // channel c of a piece lies at c * piece outputs, whatever the piece holds
            return HostPipe::Chunk{{(const char *)in_with_history + ci * piece * h->D * 8}, {(outputs(ci) * h->D + hist) * 8}, nullptr, piece * 8 * h->C};
        },
        [&](size_t ci, void *const *d_in, void *d_out, hipStream_t st) {
            for (int c = 0; c < h->C; c++) {
                d_outs[c] = (char *)d_out + (size_t)c * piece * 8;
                ph[c] = h->phase[c] + h->inc[c] * (u64)(ci * piece);  // the phase is a kernel argument: where this piece starts
            }
            return xl_launch(h, (long long)outputs(ci), d_in[0], d_outs.data(), ph.data(), st);
        },
        [&](size_t ci, const void *h_out) {
            for (int c = 0; c < h->C; c++)
                mi355_copy((char *)outs[c] + ci * piece * 8, (const char *)h_out + (size_t)c * piece * 8, outputs(ci) * 8);
        });
    if (rc) return rc;
    for (int c = 0; c < h->C; c++) h->phase[c] += h->inc[c] * (u64)noutput;
    return MI355_OK;
}
