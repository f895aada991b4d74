// clPolyphaseSynthesizer: critically sampled inverse-DFT polyphase synthesis bank as gfx950 HIP kernels -- the counterpart of
// clPolyphaseChannelizer (pfb.hip), whose item-major multiplex it consumes.  The contract is restated in include/mi355_clenabled.h; the
// reference module has no such block.
//
//     V_f[r]     = sum_q U_f[q] exp(+2 pi i r ch_map[q] / M)               U_f[q] = in[f nmap + q], T - 1 history frames first
//     y[l M + r] = sum_{p < T} g[r + M p] V_{l + T - 1 - p}[r]             one fmaf chain per component, p ascending from +0
//
// Three routes, fixed per handle at create / set_taps and named by mi355_synth_route():
//
// fused pow2     k_synth_p2<M>, M = 8 .. 4096.  256 threads, a tile = 4096 / M frames = the 4096 points of one fft_core transform in the
//                16-points-per-thread layout.  LDS: a ring of nreg = 1 + ceil((T - 1) / tile) regions of 4096 slots (32 KiB) each, then the
//                T x M taps when they still fit the 160 KiB of a CU (else they come through the caches).  So T - 1 <= 4 tiles:
//                T <= 16384 / M + 1.  A persistent workgroup owns a run of consecutive tiles; per tile it loads the tile's nmap-item frames
//                into the next region (scattered through ch_map into zeroed bins; the identity map is a straight copy), transforms them in
//                place, leaves V in natural order, and runs synthf::fir_tile: lane = r, a window of four frames sliding down the ring.
//                A run starts nreg - 1 tiles early, transform only.  Occupancy: (M = 64, T = 32) 72 KiB = two workgroups per CU,
//                (4096, 4) 128 KiB = one.
// fused mixed-radix  k_synth_mr (fft_mr.hip), M = 2^a 3^b 5^c 7^d 11^e 13^f that is not a power of two and that MrPlan takes (6, 10, 12, 20,
//                100 ... 4095; not the primes 3, 5, 7, 11, 13 themselves): the same scheme with the MrPlan passes.
// generic        k_synth_dft (a direct M-point DFT per transformed value into a workspace of the handle) + k_synth_fir: M = 1 .. 5 and 7, M with
//                a larger prime factor, arms too long for the LDS ring, MI355_SYNTH_GENERIC=1.
//
// In every route a transformed value depends on its frame only and an output is ONE chain of fmaf over exactly its T transformed frames:
// any split of a stream into calls, any tile, any 8-byte alignment gives the same bits within a route.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "common.h"
#include "fft_core.hpp"
#include "fft_mr.h"
#include "synth_fir.hpp"

namespace {

using fftc::c32;
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int kSynMaxM = 4096;
constexpr long long kSynMaxTable = 1048576;  // T * M
constexpr int kSynLds = 160 << 10;
constexpr int kSynPts = 4096;                // points per pow2 tile
constexpr int kSynMaxRegions = kSynLds / (kSynPts * 8);  // 5

struct SynP2 {
    const v2f *in;
    v2f *out;
    const float *taps;  // T x M, zero padded: tap p of phase r at p M + r
    const c32 *tw;      // exp(+2 pi i k / M)
    const int *ch_map;  // nullptr: the identity over all M channels
    int nmap, T, nreg, per;
    long long nframes, nin_items, ntiles;
};

template <int N, bool TL>
__global__ __launch_bounds__(256) void k_synth_p2(const SynP2 a)
{
    using G = fftc::Geo<N>;
    using PL = fftc::Plan<N, false>;
    constexpr int F = G::F, R0 = PL::radix(0), B0 = N / R0, RL = PL::radix(PL::NP - 1), BL = N / RL, JB = F < 4 ? F : 4;
    static_assert(G::TH == 256 && G::PTS == kSynPts, "geometry");
    extern __shared__ __attribute__((aligned(16))) c32 syn_lds[];
    const int tid = threadIdx.x;
    fftc::TwRegs<N> tw;
    fftc::load_twiddles<N, false>(tw, tid, a.tw);
    float *tl = (float *)(syn_lds + (size_t)a.nreg * kSynPts);
    if constexpr (TL)
        for (int i = tid; i < a.T * N; i += 256) tl[i] = a.taps[i];
    synthf::FirArgs fa;
    fa.M = N; fa.T = a.T; fa.F = F; fa.nreg = a.nreg; fa.rs = kSynPts; fa.m_M = (unsigned)(0x100000000ull / N);
    const long long t0 = (long long)blockIdx.x * a.per, t1 = t0 + a.per < a.ntiles ? t0 + a.per : a.ntiles;
    int reg = 0;
    for (long long t = t0 - (a.nreg - 1); t < t1; t++) {
        c32 *rgn = syn_lds + (size_t)reg * kSynPts;
        __syncthreads();  // the last tile's filter has read the region this tile overwrites; the first time: the taps are written
        // the tile's newest input frames: output frame l needs input frames l .. l + T - 1 of the history-prefixed stream
        const long long base = (t * F + (a.T - 1)) * a.nmap;
        if (a.ch_map) {
#pragma unroll
            for (int i = 0; i < 16; i++) rgn[tid + 256 * i] = fftc::mk(0.f, 0.f);
            __syncthreads();
            for (int i = tid; i < F * a.nmap; i += 256) {
                const long long gi = base + i;
                if (gi >= 0 && gi < a.nin_items) {
                    const v2f x = __builtin_nontemporal_load(a.in + gi);
                    const unsigned fr = (unsigned)i / (unsigned)a.nmap, q = (unsigned)i - fr * (unsigned)a.nmap;
                    rgn[(int)fr * N + a.ch_map[q]] = fftc::mk(x.x, x.y);
                }
            }
        } else {
            v2f x[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const long long gi = base + tid + 256 * i;
                x[i] = (v2f){0.f, 0.f};
                if (gi >= 0 && gi < a.nin_items) x[i] = __builtin_nontemporal_load(a.in + gi);
            }
#pragma unroll
            for (int i = 0; i < 16; i++) rgn[tid + 256 * i] = fftc::mk(x[i].x, x[i].y);
        }
        __syncthreads();
        c32 v[16];
#pragma unroll
        for (int q = 0; q < 16 / R0; q++) {
            const int g = tid + 256 * q, fr = g / B0, j = g % B0;
#pragma unroll
            for (int r = 0; r < R0; r++) v[q * R0 + r] = rgn[fr * N + j + r * B0];
        }
        __syncthreads();  // everyone holds its points: the transform works in place
        fftc::transform_regs<N, 1, false>(v, tw, rgn, tid);
        __syncthreads();  // the last pass' reads are done
#pragma unroll
        for (int q = 0; q < 16 / RL; q++) {
            const int g = tid + 256 * q, fr = g / BL, j = g % BL;
#pragma unroll
            for (int s = 0; s < RL; s++) rgn[fr * N + j + fftc::orev<RL>(s) * BL] = v[q * RL + s];
        }
        __syncthreads();
        if (t >= t0) {
            const long long left = a.nframes - t * F;
            const int nvalid = left < F ? (int)left : F;
            synthf::v2f *o = a.out + (size_t)t * F * N;
            if constexpr (TL) synthf::fir_tile<synthf::PadNone, JB>(syn_lds, fa, reg, tl, o, nvalid, tid, 256);
            else synthf::fir_tile<synthf::PadNone, JB>(syn_lds, fa, reg, a.taps, o, nvalid, tid, 256);
        }
        reg = reg + 1 == a.nreg ? 0 : reg + 1;
    }
}

// ---- generic route ------------------------------------------------------------------------------------------------------------
// ws[e M + r] = V of input frame j0 + e, e < nfr: M products per value, the twiddle index (r c) mod M
__global__ __launch_bounds__(256) void k_synth_dft(const c32 *__restrict__ in, c32 *__restrict__ ws, const c32 *__restrict__ twM,
                                                   const int *__restrict__ ch_map, int nmap, int M, long long j0, long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const long long e = idx / M;
        const unsigned r = (unsigned)(idx - e * M);
        const c32 *u = in + (j0 + e) * nmap;
        float sr = 0.f, si = 0.f;
        for (int q = 0; q < nmap; q++) {
            const unsigned c = ch_map ? (unsigned)ch_map[q] : (unsigned)q;
            const c32 w = twM[(r * c) % (unsigned)M], x = u[q];
            sr = fmaf(x.x, w.x, sr); sr = fmaf(-x.y, w.y, sr);
            si = fmaf(x.x, w.y, si); si = fmaf(x.y, w.x, si);
        }
        ws[idx] = fftc::mk(sr, si);
    }
}

// out[l M + r], l < nfr, from ws frames l .. l + T - 1
__global__ __launch_bounds__(256) void k_synth_fir(const c32 *__restrict__ ws, c32 *__restrict__ out, const float *__restrict__ taps, int M, int T,
                                                   long long total)
{
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const c32 *v = ws + idx + (long long)(T - 1) * M;  // frame l + T - 1, phase r
        const float *g = taps + (idx % M);
        float ax = 0.f, ay = 0.f;
        for (int p = 0; p < T; p++) {
            const float h = g[(size_t)p * M];
            const c32 x = v[-(long long)p * M];
            ax = fmaf(h, x.x, ax);
            ay = fmaf(h, x.y, ay);
        }
        out[idx] = fftc::mk(ax, ay);
    }
}

// ---- bookkeeping shared by _plan and the handle ---------------------------------------------------------------------------------
int syn_check(int K, int M, int nmap)
{
    MI355_REQUIRE(M >= 1, "num_channels must be >= 1");
    MI355_REQUIRE(K >= 1, "at least one tap");
    if (M > kSynMaxM) {
        mi355_set_error("clPolyphaseSynthesizer: %d channels, the limit is %d", M, kSynMaxM);
        return MI355_ERR_UNSUPPORTED;
    }
    MI355_REQUIRE(nmap >= 1 && nmap <= M, "nmap outside 1 .. num_channels");
    const long long T = ((long long)K + M - 1) / M;
    if (T * M > kSynMaxTable) {
        mi355_set_error("clPolyphaseSynthesizer: %lld taps per arm x %d arms = %lld table entries, the limit is %lld", T, M, T * M, kSynMaxTable);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

inline int syn_T(int K, int M) { return (int)(((long long)K + M - 1) / M); }

enum { kRouteGeneric = 0, kRoutePow2 = 1, kRouteMr = 2 };

}  // namespace

struct mi355_synth {
    mi355_ctx *ctx = nullptr;
    int M = 1, K = 0, T = 0, nmap = 1;
    bool ident = true;                // ch_map = 0 .. M-1
    bool force_generic = false;       // MI355_SYNTH_GENERIC at create
    std::vector<float> taps_host;
    mi355_tables taps;                // T x M, zero padded
    void *d_tw = nullptr;             // exp(+2 pi i k / M), k < M
    int *d_map = nullptr;             // nmap entries (also for the identity: the generic kernel of a partial identity needs none, but the table is tiny)
    int route = kRouteGeneric;
    std::string route_name = "generic";
    int nreg = 0, taps_lds = 0, lds_bytes = 0;  // pow2
    MrPlan plan;                      // mixed radix (plan.n = 0: none)
    MrSynthGeo mg;
    DevBuf ws;                        // generic route: transformed frames of one piece
    DevBuf d_in, d_out;               // host path staging
    std::mutex lock;
};

namespace {

constexpr long long kSynHostChunk = 1ll << 20;  // output items per staging piece of the host-pointer path
constexpr long long kSynWsItems = 4ll << 20;    // generic route: transformed values per piece (32 MiB)

template <int N, bool TL> int p2_attr()
{
    MI355_HIP(hipFuncSetAttribute((const void *)k_synth_p2<N, TL>, hipFuncAttributeMaxDynamicSharedMemorySize, kSynLds));
    return MI355_OK;
}

#define SYN_P2_SIZES(X) X(8) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096)

// the route of a handle; caller has set the device
int syn_choose(mi355_synth *h)
{
    const int M = h->M, T = h->T;
    h->route = kRouteGeneric;
    h->route_name = "generic";
    if (h->force_generic) return MI355_OK;
    const bool pow2 = (M & (M - 1)) == 0;
    char name[96];
    if (pow2 && M >= 8) {
        const int F = kSynPts / M;
        const long long nreg = 1 + ((long long)T - 1 + F - 1) / F;
        if (nreg > kSynMaxRegions) return MI355_OK;  // arms too long for the ring
        const long long ring = nreg * kSynPts * 8, tap_bytes = (long long)T * M * 4;
        h->nreg = (int)nreg;
        const char *tg = getenv("MI355_SYNTH_TAPS_GLOBAL");  // comparison aid: the taps through the caches although they fit the LDS
        h->taps_lds = ring + tap_bytes <= kSynLds && !(tg && atoi(tg) > 0);
        h->lds_bytes = (int)(ring + (h->taps_lds ? tap_bytes : 0));
        if (h->lds_bytes > (48 << 10)) {
            int rc = MI355_OK;
#define X(N) if (M == N) rc = h->taps_lds ? p2_attr<N, true>() : p2_attr<N, false>();
            SYN_P2_SIZES(X)
#undef X
            if (rc) return rc;
        }
        h->route = kRoutePow2;
        snprintf(name, sizeof name, "fused pow2 M=%d T=%d tile=%d%s", M, T, F, !h->taps_lds && ring + tap_bytes <= kSynLds ? " taps=global" : "");
        h->route_name = name;
        return MI355_OK;
    }
    if (h->plan.n == M && mi355_fft_mr_synth_ok(h->plan, 1, M, T, &h->mg)) {
        h->route = kRouteMr;
        snprintf(name, sizeof name, "fused mixed-radix M=%d T=%d tile=%d", M, T, h->mg.frames);
        h->route_name = name;
    }
    return MI355_OK;
}

// caller holds h->lock (or is create) and has set the device
int syn_upload(mi355_synth *h, const float *taps, int K)
{
    MI355_REQUIRE(taps != nullptr, "taps is NULL");
    int rc = syn_check(K, h->M, h->nmap);
    if (rc) return rc;
    const int T = syn_T(K, h->M);
    std::vector<float> pad((size_t)T * h->M, 0.f);
    for (int k = 0; k < K; k++) pad[k] = taps[k];  // g[r + M p] at p M + r: the padded taps as they are
    rc = h->taps.publish(h->ctx, pad.data(), pad.size() * sizeof(float), "mi355_synth: tap");
    if (rc) return rc;
    h->K = K;
    h->T = T;
    h->taps_host.assign(taps, taps + K);
    rc = syn_choose(h);
    if (rc) return rc;
    mi355_log(h->ctx, MI355_LOG_INFO, "clPolyphaseSynthesizer: %d channels, %d of them fed, %d taps (%d per arm): %s", h->M, h->nmap, K, T,
              h->route_name.c_str());
    return MI355_OK;
}

// caller holds h->lock and has set the device
int syn_launch(mi355_synth *h, long long nframes, const void *in, void *out, hipStream_t st)
{
    const int M = h->M, T = h->T;
    const int cus = mi355_cus(h->ctx);
    const int *map = h->ident ? nullptr : h->d_map;
    const float *d_taps = (const float *)h->taps.current();
    if (h->route == kRouteMr) return mi355_fft_mr_synth_launch(h->plan, h->mg, h->ctx, in, out, d_taps, map, h->nmap, T, nframes, st);
    if (h->route == kRoutePow2) {
        const int F = kSynPts / M;
        int per_cu = kSynLds / h->lds_bytes;
        if (per_cu > 4) per_cu = 4;
        const long long ntiles = (nframes + F - 1) / F, cap = (long long)cus * per_cu;
        // a run re-transforms nreg - 1 tiles: runs of at least four times that while there are tiles to share out
        const long long minrun = h->nreg > 1 ? 4LL * (h->nreg - 1) : 1;
        long long grid = (ntiles + minrun - 1) / minrun;
        if (grid > cap) grid = cap;
        const long long per = (ntiles + grid - 1) / grid;
        grid = (ntiles + per - 1) / per;
        SynP2 a;
        a.in = (const v2f *)in;
        a.out = (v2f *)out;
        a.taps = d_taps;
        a.tw = (const c32 *)h->d_tw;
        a.ch_map = map;
        a.nmap = h->nmap;
        a.T = T;
        a.nreg = h->nreg;
        a.per = (int)per;
        a.nframes = nframes;
        a.nin_items = ((long long)T - 1 + nframes) * h->nmap;
        a.ntiles = ntiles;
#define X(N)                                                                                                                     \
    if (M == N) {                                                                                                                \
        if (h->taps_lds) hipLaunchKernelGGL((k_synth_p2<N, true>), dim3((unsigned)grid), dim3(256), (size_t)h->lds_bytes, st, a); \
        else hipLaunchKernelGGL((k_synth_p2<N, false>), dim3((unsigned)grid), dim3(256), (size_t)h->lds_bytes, st, a);            \
    }
        SYN_P2_SIZES(X)
#undef X
        MI355_HIP(hipGetLastError());
        return MI355_OK;
    }
    // generic: pieces of frames whose transformed values (T - 1 older frames included) fit the workspace
    long long piece = kSynWsItems / M - (T - 1);
    if (piece < 1) piece = 1;
    if (piece > nframes) piece = nframes;
    const int rc = h->ws.reserve((size_t)(T - 1 + piece) * M * 8);
    if (rc) return rc;
    for (long long l0 = 0; l0 < nframes; l0 += piece) {
        const long long n = nframes - l0 < piece ? nframes - l0 : piece;
        const long long tv = (T - 1 + n) * M, to = n * M;
        long long g1 = (tv + 255) / 256, g2 = (to + 255) / 256;
        if (g1 > (long long)cus * 32) g1 = (long long)cus * 32;
        if (g2 > (long long)cus * 32) g2 = (long long)cus * 32;
        hipLaunchKernelGGL(k_synth_dft, dim3((unsigned)g1), dim3(256), 0, st, (const c32 *)in, (c32 *)h->ws.get(), (const c32 *)h->d_tw, map, h->nmap, M, l0,
                           tv);
        hipLaunchKernelGGL(k_synth_fir, dim3((unsigned)g2), dim3(256), 0, st, (const c32 *)h->ws.get(), (c32 *)out + l0 * M, d_taps, M, T, to);
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

int syn_args(const mi355_synth *h, long long nframes, const void *in, void *out)
{
    MI355_REQUIRE(nframes >= 0, "nframes is negative");
    if (nframes == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0, "buffers must be 8-byte aligned");
    if (nframes > (1ll << 44) / h->M) {
        mi355_set_error("clPolyphaseSynthesizer: %lld frames of %d outputs in one call", nframes, h->M);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

bool syn_overlap(const void *in, long long in_items, const void *out, long long out_items)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    return a < b + (uintptr_t)out_items * 8 && b < a + (uintptr_t)in_items * 8;
}

}  // namespace

extern "C" int mi355_synth_plan(int ntaps, int num_channels, int nmap, long long nframes, int *taps_per_arm, long long *ninput_items,
                                long long *noutput_items)
{
    if (taps_per_arm) *taps_per_arm = 0;
    if (ninput_items) *ninput_items = 0;
    if (noutput_items) *noutput_items = 0;
    const int rc = syn_check(ntaps, num_channels, nmap);
    if (rc) return rc;
    MI355_REQUIRE(nframes >= 0, "nframes is negative");
    if (nframes > (1ll << 44) / num_channels) {
        mi355_set_error("clPolyphaseSynthesizer: %lld frames of %d outputs in one call", nframes, num_channels);
        return MI355_ERR_UNSUPPORTED;
    }
    const int T = syn_T(ntaps, num_channels);
    if (taps_per_arm) *taps_per_arm = T;
    if (ninput_items) *ninput_items = ((long long)T - 1 + nframes) * nmap;
    if (noutput_items) *noutput_items = nframes * num_channels;
    return MI355_OK;
}

extern "C" int mi355_synth_create(mi355_ctx *ctx, const float *taps, int ntaps, int num_channels, const int *ch_map, int nmap, mi355_synth **out)
{
    if (out) *out = nullptr;
    // everything that can be told without a device comes first
    int rc = syn_check(ntaps, num_channels, nmap);
    if (rc) return rc;
    MI355_REQUIRE(taps != nullptr, "taps is NULL");
    const int M = num_channels;
    std::vector<int> map(nmap);
    bool ident = nmap == M;
    {
        std::vector<char> seen(M, 0);
        for (int q = 0; q < nmap; q++) {
            const int c = ch_map ? ch_map[q] : q;  // NULL: slot q feeds channel q
            MI355_REQUIRE(c >= 0 && c < M, "ch_map entry outside [0, num_channels)");
            MI355_REQUIRE(!seen[c], "ch_map entries must be distinct");
            seen[c] = 1;
            map[q] = c;
            if (c != q) ident = false;
        }
    }
    MI355_REQUIRE(ctx && out, "NULL argument");
    mi355_synth *h = new (std::nothrow) mi355_synth();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->M = M; h->nmap = nmap; h->ident = ident;
    const char *e = getenv("MI355_SYNTH_GENERIC");  // the generic route for every handle made while it is set
    h->force_generic = e && atoi(e) > 0;
    auto fail = [&](int code) {
        mi355_synth_destroy(h);
        return code;
    };
    if (hipSetDevice(ctx->device) != hipSuccess) {
        mi355_set_error("mi355_synth_create: hipSetDevice failed");
        return fail(MI355_ERR_HIP);
    }
    std::vector<float> tw((size_t)2 * M);
    for (int k = 0; k < M; k++) {
        const double a = 2.0 * M_PI * (double)k / (double)M;
        tw[2 * k] = (float)cos(a);
        tw[2 * k + 1] = (float)sin(a);
    }
    if (hipMalloc(&h->d_tw, tw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_NOMEM);
    if (hipMalloc((void **)&h->d_map, (size_t)nmap * sizeof(int)) != hipSuccess) return fail(MI355_ERR_NOMEM);
    if (mi355_upload(ctx, h->d_tw, tw.data(), tw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_HIP);
    if (mi355_upload(ctx, h->d_map, map.data(), (size_t)nmap * sizeof(int)) != hipSuccess) return fail(MI355_ERR_HIP);
    if ((M & (M - 1)) != 0 && !h->force_generic) {
        std::vector<float> mtw;
        if (mi355_fft_mr_plan(M, 1, 0, &h->plan, &mtw)) {
            const size_t bytes = (mtw.empty() ? 2 : mtw.size()) * sizeof(float);
            if (hipMalloc(&h->plan.d_tw, bytes) != hipSuccess) return fail(MI355_ERR_NOMEM);
            if (!mtw.empty() && mi355_upload(ctx, h->plan.d_tw, mtw.data(), mtw.size() * sizeof(float)) != hipSuccess) return fail(MI355_ERR_HIP);
        } else {
            h->plan.n = 0;
        }
    }
    rc = syn_upload(h, taps, ntaps);
    if (rc) return fail(rc);
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_synth_destroy(mi355_synth *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->taps.release();
    if (h->d_tw) (void)hipFree(h->d_tw);
    if (h->d_map) (void)hipFree(h->d_map);
    if (h->plan.d_tw) (void)hipFree(h->plan.d_tw);
    for (DevBuf *b : {&h->ws, &h->d_in, &h->d_out}) b->release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_synth_set_taps(mi355_synth *h, const float *taps, int ntaps)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return syn_upload(h, taps, ntaps);
}

extern "C" int mi355_synth_ntaps(const mi355_synth *h) { return h ? h->K : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_synth_taps_per_arm(const mi355_synth *h) { return h ? h->T : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_synth_num_channels(const mi355_synth *h) { return h ? h->M : MI355_ERR_INVALID_ARG; }
extern "C" int mi355_synth_nmap(const mi355_synth *h) { return h ? h->nmap : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_synth_get_taps(const mi355_synth *h, float *taps_out, int cap)
{
    MI355_REQUIRE(h && taps_out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_synth *>(h)->lock);
    MI355_REQUIRE(cap >= h->K, "taps_out too small");
    memcpy(taps_out, h->taps_host.data(), h->taps_host.size() * sizeof(float));
    return h->K;
}

// valid until the next set_taps or destroy of this handle
extern "C" const char *mi355_synth_route(const mi355_synth *h) { return h ? h->route_name.c_str() : ""; }

extern "C" int mi355_synth_work_dev(mi355_synth *h, long long nframes, const void *in_with_history, void *out, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = syn_args(h, nframes, in_with_history, out);
    if (rc || nframes == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_REQUIRE(!syn_overlap(in_with_history, ((long long)h->T - 1 + nframes) * h->nmap, out, nframes * h->M),
                  "clPolyphaseSynthesizer does not work in place: in and out overlap");
    MI355_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = mi355_pick_stream(h->ctx, stream);
    const int rc2 = syn_launch(h, nframes, in_with_history, out, st);
    return rc2 ? rc2 : h->taps.used(st);  // this table may be released behind this launch
}

extern "C" int mi355_synth_work(mi355_synth *h, long long nframes, const void *in_with_history, void *out)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = syn_args(h, nframes, in_with_history, out);
    if (rc || nframes == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_REQUIRE(!syn_overlap(in_with_history, ((long long)h->T - 1 + nframes) * h->nmap, out, nframes * h->M),
                  "clPolyphaseSynthesizer does not work in place: in and out overlap");
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of about kSynHostChunk outputs; each piece re-sends its T - 1 frames of history
    const long long piece = mi355_piece_units(kSynHostChunk / h->M, nframes);
    if ((rc = h->d_in.reserve((size_t)(h->T - 1 + piece) * h->nmap * 8))) return rc;
    if ((rc = h->d_out.reserve((size_t)piece * h->M * 8))) return rc;
    return mi355_pageable_run(h->ctx, nframes, piece, [&](long long l0, long long n, hipStream_t st) -> int {
        MI355_HIP(hipMemcpyAsync(h->d_in.get(), (const char *)in_with_history + l0 * h->nmap * 8, (size_t)(h->T - 1 + n) * h->nmap * 8,
                                 hipMemcpyHostToDevice, st));
        const int lrc = syn_launch(h, n, h->d_in.get(), h->d_out.get(), st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + l0 * h->M * 8, h->d_out.get(), (size_t)n * h->M * 8, hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
}
