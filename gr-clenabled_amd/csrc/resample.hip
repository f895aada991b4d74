// clRationalResampler: polyphase FIR with interpolation L and decimation M as gfx950 HIP kernels.  The contract is GNU Radio's
// rational_resampler_ccf / ccc (M = 1: interp_fir_filter), restated in include/mi355_clenabled.h; the reference module has no
// such block.
//
//     q = c + m M;  p = q mod L;  b = q div L;   y[m] = sum_j hp[p + L j] in[nt - 1 + b - j]  =  sum_i rev[p][i] in[b + i]
//
// with rev[p][i] = hp[p + L (nt - 1 - i)]: the device table holds every arm reversed, so an output is a dot product of its arm
// with the ascending window in[b .. b + nt).
//
// k_rs_lds    one output per lane, consecutive lanes consecutive outputs.  A workgroup keeps the whole arm table in LDS
//             ([arm][i], the arm stride padded to an odd count of entries: lanes of a wave sit on different arms, stepping by
//             M mod L, and an odd stride puts different arms on different banks) and walks tiles of `tile` outputs: the input
//             span of a tile is staged in LDS with 8-byte loads, four per thread in flight before the first LDS write (any
//             8-byte alignment of the buffer takes the same path), then every lane reads its window from LDS (ds_read_b64 per
//             sample, a broadcast where L > M).  Persistent over tiles, so the table is loaded once per workgroup.
// k_rs_interp M = 1 and 4 <= L <= 16, at most 40 taps per arm (pulse shaping): lanes over input positions, the window in registers,
//             the arms in a uniform loop with broadcast LDS taps, the outputs turned through LDS -- see the kernel.
// k_rs_plain  one output per lane, table and samples from global memory: everything the LDS form cannot hold (a table or a
//             tile span beyond 64 KiB: huge L, huge M / L).
// All run ONE chain of fmaf per component over i = 0 .. nt-1 and nothing else, so an output's bits depend on its arm and its
// window only: any split of a stream into calls, any tile, any alignment gives the same bits, and no product touches a sample
// outside the window.  Which kernel serves a handle is decided at create / set_taps.
#include <cstdint>
#include <vector>
#include "common.h"

namespace {

typedef float2 c32;
typedef float v2f __attribute__((ext_vector_type(2)));  // the nontemporal builtins take vector types only

constexpr int kRsThreads = 256;
constexpr int kRsMaxRate = 65536;
constexpr long long kRsMaxTable = 1048576;  // nt * L entries
constexpr int kRsLdsBytes = 64 << 10;       // never more: no hipFuncSetAttribute needed

template <bool CTAPS>
__device__ __forceinline__ void rs_step(float &ax, float &ay, const float *__restrict__ arm, int i, const c32 s)
{
    if constexpr (CTAPS) {
        const float hr = arm[2 * i], hi = arm[2 * i + 1];
        ax = fmaf(hr, s.x, ax); ax = fmaf(-hi, s.y, ax);
        ay = fmaf(hr, s.y, ay); ay = fmaf(hi, s.x, ay);
    } else {
        const float h = arm[i];
        ax = fmaf(h, s.x, ax);
        ay = fmaf(h, s.y, ay);
    }
}

// rev: [L][nt] entries (float, or float pairs for complex taps).  LDS: the table at an arm stride of ntp entries, then the tile's
// input span from float x_off on.  `tile` outputs per tile, a multiple of kRsThreads; rs_choose() sized it so that the span of any
// tile fits the LDS the launch asks for.
template <bool CTAPS>
__global__ __launch_bounds__(kRsThreads) void k_rs_lds(const c32 *__restrict__ in, c32 *__restrict__ out, const float *__restrict__ rev,
                                                       int L, int M, int nt, int ntp, int phase, long long n_out, int tile, int x_off /* floats */)
{
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    constexpr int E = CTAPS ? 2 : 1;
    float *const tl = rs_lds;
    c32 *const xl = (c32 *)(rs_lds + x_off);
    const int tid = threadIdx.x;
    for (int i = tid; i < L * nt; i += kRsThreads) {
        const int p = i / nt, k = i - p * nt;
        if constexpr (CTAPS) ((float2 *)tl)[p * ntp + k] = ((const float2 *)rev)[i];
        else tl[p * ntp + k] = rev[i];
    }
    const long long ntiles = (n_out + tile - 1) / tile;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long o0 = t * tile, left = n_out - o0;
        const int no = left < tile ? (int)left : tile;
        const long long q0 = (long long)phase + o0 * M;
        const long long b0 = q0 / L;
        const unsigned r0 = (unsigned)(q0 - b0 * L);                       // < L
        const int span = (int)((r0 + (unsigned)(no - 1) * (unsigned)M) / (unsigned)L) + nt;  // samples in[b0 .. b0 + span) and no more
        const c32 *__restrict__ src = in + b0;
        __syncthreads();  // the previous tile's reads are done; the first time: the table is written
        for (int s0 = 0; s0 < span; s0 += 4 * kRsThreads) {
            c32 v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int s = s0 + j * kRsThreads + tid;
                if (s < span) {
                    const v2f a = __builtin_nontemporal_load((const v2f *)(src + s));
                    v[j] = make_float2(a.x, a.y);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int s = s0 + j * kRsThreads + tid;
                if (s < span) xl[s] = v[j];
            }
        }
        __syncthreads();
        for (int o = tid; o < no; o += kRsThreads) {
            const unsigned r = r0 + (unsigned)o * (unsigned)M;             // < 65536 + 2048 * 65536
            const unsigned bo = r / (unsigned)L, p = r - bo * (unsigned)L;
            const float *arm = tl + (size_t)p * ntp * E;
            const c32 *x = xl + bo;
            float ax = 0.f, ay = 0.f;
#pragma unroll 4
            for (int i = 0; i < nt; i++) rs_step<CTAPS>(ax, ay, arm, i, x[i]);
            __builtin_nontemporal_store((v2f){ax, ay}, (v2f *)(out + o0 + o));
        }
    }
}

// M = 1, L = 4 .. 16: lanes run over INPUT positions b, a uniform loop runs over the L arms.  A lane reads its window in[b .. b + nt) from
// the staged tile into registers once and reuses it for all L outputs q = b L + p; the arm, and with it every tap, is wave-uniform:
// 16-byte LDS reads at one address for the whole wave (a broadcast), four real taps each.  The L outputs of a lane are L apart from
// the next lane's, so the tile's outputs are turned through LDS (one padding unit per 16, which spreads the stride-L stores over
// the banks) and leave as whole lines.
// NTB: registers for the window, nt rounded up to a multiple of 8.  The table in LDS pads every arm with zeros to NTB and the window
// registers past nt hold zeros the kernel put there itself, so the chain runs NTB steps with no branch: the padded steps add
// 0 * 0 and never see a sample outside the window.
constexpr int kRiTile = kRsThreads;      // input positions per tile
constexpr int kRiMinL = 4, kRiMaxL = 16, kRiMaxNt = 40;  // at L = 2 the general kernel ties it (measured); L = 3 was not measured
typedef float v4f __attribute__((ext_vector_type(4)));
__host__ __device__ inline int ri_pad(int o) { return o + (o >> 4); }

template <bool CTAPS, int NTB>
__global__ __launch_bounds__(kRsThreads) void k_rs_interp(const c32 *__restrict__ in, c32 *__restrict__ out, const float *__restrict__ rev,
                                                          int L, int nt, int phase, long long n_out, int x_off, int y_off /* floats */)
{
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    constexpr int E = CTAPS ? 2 : 1;
    float *const tl = rs_lds;                 // [L][NTB] entries
    c32 *const xl = (c32 *)(rs_lds + x_off);  // kRiTile + NTB samples
    c32 *const yl = (c32 *)(rs_lds + y_off);
    const int tid = threadIdx.x;
    for (int i = tid; i < L * NTB; i += kRsThreads) {
        const int p = i / NTB, k = i - p * NTB;
#pragma unroll
        for (int e = 0; e < E; e++) tl[i * E + e] = k < nt ? rev[((size_t)p * nt + k) * E + e] : 0.f;
    }
    const long long bcount = ((long long)phase + n_out - 1) / L + 1;  // input positions b = 0 .. bcount-1 carry outputs
    const long long ntiles = (bcount + kRiTile - 1) / kRiTile;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long b0 = t * kRiTile, left = bcount - b0;
        const int nb = left < kRiTile ? (int)left : kRiTile;
        const int span = nb + nt - 1;  // samples in[b0 .. b0 + span): the last one is item needed - 1 at the most
        const c32 *__restrict__ src = in + b0;
        __syncthreads();  // the previous tile's reads of both LDS regions are done; the first time: the table is written
        for (int s = tid; s < span; s += kRsThreads) {
            const v2f a = __builtin_nontemporal_load((const v2f *)(src + s));
            xl[s] = make_float2(a.x, a.y);
        }
        __syncthreads();
        if (tid < nb) {
            c32 x[NTB];
#pragma unroll
            for (int i = 0; i < NTB; i++) {
                const c32 v = xl[tid + i];  // inside the LDS region whatever it holds; past the window it is dropped here
                x[i] = i < nt ? v : make_float2(0.f, 0.f);
            }
            for (int p = 0; p < L; p++) {
                const v4f *arm = (const v4f *)(tl + (size_t)p * NTB * E);  // uniform
                float ax = 0.f, ay = 0.f;
#pragma unroll
                for (int i0 = 0; i0 < NTB; i0 += 4) {
                    if constexpr (CTAPS) {
                        const v4f h0 = arm[i0 / 2], h1 = arm[i0 / 2 + 1];
                        const float hv[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
                        for (int k = 0; k < 4; k++) rs_step<true>(ax, ay, hv, k, x[i0 + k]);
                    } else {
                        const v4f h0 = arm[i0 / 4];
                        const float hv[4] = {h0.x, h0.y, h0.z, h0.w};
#pragma unroll
                        for (int k = 0; k < 4; k++) rs_step<false>(ax, ay, hv, k, x[i0 + k]);
                    }
                }
                yl[ri_pad(tid * L + p)] = make_float2(ax, ay);
            }
        }
        __syncthreads();
        const long long m0 = b0 * L - phase;  // output index of the tile's (b0, arm 0)
        for (int o = tid; o < nb * L; o += kRsThreads) {
            const long long m = m0 + o;
            if (m >= 0 && m < n_out) {
                const c32 v = yl[ri_pad(o)];
                __builtin_nontemporal_store((v2f){v.x, v.y}, (v2f *)(out + m));
            }
        }
    }
}

template <bool CTAPS>
__global__ __launch_bounds__(kRsThreads) void k_rs_plain(const c32 *__restrict__ in, c32 *__restrict__ out, const float *__restrict__ rev,
                                                         int L, int M, int nt, int phase, long long n_out)
{
    constexpr int E = CTAPS ? 2 : 1;
    for (long long m = (long long)blockIdx.x * kRsThreads + threadIdx.x; m < n_out; m += (long long)gridDim.x * kRsThreads) {
        const long long q = (long long)phase + m * M;
        const long long b = q / L;
        const int p = (int)(q - b * L);
        const float *__restrict__ arm = rev + (size_t)p * nt * E;
        const c32 *__restrict__ x = in + b;
        float ax = 0.f, ay = 0.f;
#pragma unroll 4
        for (int i = 0; i < nt; i++) rs_step<CTAPS>(ax, ay, arm, i, x[i]);
        out[m] = make_float2(ax, ay);
    }
}

// ---- bookkeeping shared by _plan, _noutput_for and the handle ----------------------------------------------------------
int rs_check(int L, int M, int K)
{
    MI355_REQUIRE(L >= 1, "interpolation must be >= 1");
    MI355_REQUIRE(M >= 1, "decimation must be >= 1");
    MI355_REQUIRE(K >= 1, "at least one tap");
    if (L > kRsMaxRate || M > kRsMaxRate) {
        mi355_set_error("clRationalResampler: interpolation %d / decimation %d beyond %d", L, M, kRsMaxRate);
        return MI355_ERR_UNSUPPORTED;
    }
    const long long nt = ((long long)K + L - 1) / L;
    if (nt * L > kRsMaxTable) {
        mi355_set_error("clRationalResampler: %lld taps per arm x %d arms = %lld table entries, the limit is %lld", nt, L, nt * L, kRsMaxTable);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

inline int rs_nt(int L, int K) { return (int)(((long long)K + L - 1) / L); }

inline long long rs_needed(int L, int M, int nt, int c, long long n) { return n == 0 ? 0 : nt + (c + (n - 1) * M) / L; }

}  // namespace

struct mi355_resampler {
    mi355_ctx *ctx = nullptr;
    int L = 1, M = 1, K = 0, nt = 0, complex_taps = 0;
    int phase = 0;                    // host state: a pure function of the outputs produced so far
    std::vector<float> taps_host;     // K floats, or 2 K for complex taps
    mi355_tables rev;                 // [L][nt] reversed arms
    bool lds = false;                 // k_rs_lds serves the handle (else k_rs_plain); fixed by set_taps
    int interp = 0;                   // k_rs_interp with this many window registers serves it instead (0: no)
    int ntp = 0, tile = 0, x_off = 0, y_off = 0, lds_bytes = 0, wg_per_cu = 1;
    DevBuf d_in, d_out;  // host path staging
    std::mutex lock;
};

namespace {

constexpr long long kRsHostChunk = 1ll << 20;  // items per staging piece of the host-pointer path (the larger of its two sides)

// the kernel of a handle: the LDS form when the table and the span of a tile of at least kRsThreads outputs fit 64 KiB; tiles as
// large as 40 KiB allow (four workgroups per CU), up to 2048 outputs
void rs_choose(mi355_resampler *h)
{
    const int E = h->complex_taps ? 2 : 1;
    h->lds = false;
    h->interp = 0;
    const char *e = getenv("MI355_RESAMPLER_PLAIN");  // tuning aid: the fallback kernel for every handle made while it is set
    if (e && atoi(e) > 0) return;
    const char *g = getenv("MI355_RESAMPLER_GENERAL");  // tuning aid: k_rs_lds also where k_rs_interp would serve
    if (h->M == 1 && h->L >= kRiMinL && h->L <= kRiMaxL && h->nt <= kRiMaxNt && !(g && atoi(g) > 0)) {
        h->interp = (h->nt + 7) / 8 * 8;
        h->x_off = h->L * h->interp * E;                          // floats: the table, a multiple of 8
        h->y_off = h->x_off + 2 * (kRiTile + h->interp);          // then the samples a lane may read, then the outputs
        h->lds_bytes = (h->y_off + 2 * (ri_pad(kRiTile * h->L) + 1)) * 4;
        const int k = (160 << 10) / h->lds_bytes;
        h->wg_per_cu = k > 8 ? 8 : k;
        return;
    }
    const long long ntp = h->nt | 1;
    const long long tap_floats = ((long long)h->L * ntp * E + 3) & ~3ll;  // the samples start on 16 bytes
    auto bytes = [&](int tile) {
        const long long span = ((long long)(h->L - 1) + (long long)(tile - 1) * h->M) / h->L + h->nt;
        return tap_floats * 4 + span * 8;
    };
    int tile = 0;
    for (int t = 2048; t >= kRsThreads; t >>= 1)
        if (bytes(t) <= (40 << 10)) { tile = t; break; }
    if (!tile && bytes(kRsThreads) <= kRsLdsBytes) tile = kRsThreads;
    if (!tile) return;
    h->lds = true;
    h->ntp = (int)ntp; h->tile = tile; h->x_off = (int)tap_floats; h->lds_bytes = (int)bytes(tile);
    const int k = (160 << 10) / h->lds_bytes;
    h->wg_per_cu = k > 8 ? 8 : (k < 1 ? 1 : k);
}

// caller holds h->lock (or is create) and has set the device
int rs_upload(mi355_resampler *h, const void *taps, int K)
{
    MI355_REQUIRE(taps != nullptr, "taps is NULL");
    const int rc = rs_check(h->L, h->M, K);
    if (rc) return rc;
    const int E = h->complex_taps ? 2 : 1, nt = rs_nt(h->L, K), L = h->L;
    const float *t = (const float *)taps;
    std::vector<float> rev((size_t)L * nt * E, 0.f);
    for (int k = 0; k < K; k++) {  // h[k] = hp[p + L j] -> rev[p][nt - 1 - j]
        const int p = k % L, j = k / L;
        for (int e = 0; e < E; e++) rev[((size_t)p * nt + (nt - 1 - j)) * E + e] = t[(size_t)k * E + e];
    }
    const int rc2 = h->rev.publish(h->ctx, rev.data(), rev.size() * sizeof(float), "mi355_resampler: table");
    if (rc2) return rc2;
    h->K = K; h->nt = nt;
    h->taps_host.assign(t, t + (size_t)K * E);
    rs_choose(h);
    if (h->interp)
        mi355_log(h->ctx, MI355_LOG_INFO, "clRationalResampler: interpolation %d, decimation %d, %d %s taps (%d per arm): k_rs_interp, %d window registers, %d bytes of LDS",
                  h->L, h->M, K, h->complex_taps ? "complex" : "real", nt, h->interp, h->lds_bytes);
    else if (h->lds)
        mi355_log(h->ctx, MI355_LOG_INFO, "clRationalResampler: interpolation %d, decimation %d, %d %s taps (%d per arm): k_rs_lds, tiles of %d outputs, %d bytes of LDS",
                  h->L, h->M, K, h->complex_taps ? "complex" : "real", nt, h->tile, h->lds_bytes);
    else
        mi355_log(h->ctx, MI355_LOG_INFO, "clRationalResampler: interpolation %d, decimation %d, %d %s taps (%d per arm): k_rs_plain (fallback)",
                  h->L, h->M, K, h->complex_taps ? "complex" : "real", nt);
    return MI355_OK;
}

// caller holds h->lock and has set the device; phase: of output 0 of this launch
int rs_launch(mi355_resampler *h, long long n, int phase, const void *in, void *out, hipStream_t st)
{
    const c32 *x = (const c32 *)in;
    c32 *y = (c32 *)out;
    const float *d_rev = (const float *)h->rev.current();
    const int cus = mi355_cus(h->ctx);
    if (h->interp) {
        const long long bcount = ((long long)phase + n - 1) / h->L + 1, tiles = (bcount + kRiTile - 1) / kRiTile, cap = (long long)cus * h->wg_per_cu;
        const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
#define RI_CASE(CT, NTB)                                                                                                          \
    if ((h->complex_taps != 0) == CT && h->interp == NTB)                                                                         \
        hipLaunchKernelGGL((k_rs_interp<CT, NTB>), grid, dim3(kRsThreads), (size_t)h->lds_bytes, st, x, y, d_rev, h->L, h->nt, phase, n, h->x_off, h->y_off);
        RI_CASE(false, 8) RI_CASE(false, 16) RI_CASE(false, 24) RI_CASE(false, 32) RI_CASE(false, 40)
        RI_CASE(true, 8) RI_CASE(true, 16) RI_CASE(true, 24) RI_CASE(true, 32) RI_CASE(true, 40)
#undef RI_CASE
    } else if (h->lds) {
        const long long tiles = (n + h->tile - 1) / h->tile, cap = (long long)cus * h->wg_per_cu;
        const dim3 grid((unsigned)(tiles < cap ? tiles : cap));
        if (h->complex_taps)
            hipLaunchKernelGGL(k_rs_lds<true>, grid, dim3(kRsThreads), (size_t)h->lds_bytes, st, x, y, d_rev, h->L, h->M, h->nt, h->ntp, phase, n, h->tile, h->x_off);
        else
            hipLaunchKernelGGL(k_rs_lds<false>, grid, dim3(kRsThreads), (size_t)h->lds_bytes, st, x, y, d_rev, h->L, h->M, h->nt, h->ntp, phase, n, h->tile, h->x_off);
    } else {
        const long long blocks = (n + kRsThreads - 1) / kRsThreads, cap = (long long)cus * 32;
        const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
        if (h->complex_taps)
            hipLaunchKernelGGL(k_rs_plain<true>, grid, dim3(kRsThreads), 0, st, x, y, d_rev, h->L, h->M, h->nt, phase, n);
        else
            hipLaunchKernelGGL(k_rs_plain<false>, grid, dim3(kRsThreads), 0, st, x, y, d_rev, h->L, h->M, h->nt, phase, n);
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

int rs_args(mi355_resampler *h, long long n, const void *in, void *out)
{
    MI355_REQUIRE(n >= 0, "noutput is negative");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0, "buffers must be 8-byte aligned");
    if (n > (1ll << 44)) {
        mi355_set_error("clRationalResampler: %lld outputs in one call", n);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

bool rs_overlap(const void *in, long long in_items, const void *out, long long out_items)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    return a < b + (uintptr_t)out_items * 8 && b < a + (uintptr_t)in_items * 8;
}

}  // namespace

extern "C" int mi355_resampler_plan(int interpolation, int decimation, int ntaps, int phase, long long noutput, int *taps_per_arm,
                                    long long *consumed, long long *needed, int *phase_after)
{
    if (taps_per_arm) *taps_per_arm = 0;
    if (consumed) *consumed = 0;
    if (needed) *needed = 0;
    if (phase_after) *phase_after = 0;
    const int rc = rs_check(interpolation, decimation, ntaps);
    if (rc) return rc;
    MI355_REQUIRE(phase >= 0 && phase < interpolation, "phase outside [0, interpolation)");
    MI355_REQUIRE(noutput >= 0, "noutput is negative");
    if (noutput > (1ll << 44)) {
        mi355_set_error("clRationalResampler: %lld outputs in one call", noutput);
        return MI355_ERR_UNSUPPORTED;
    }
    const int nt = rs_nt(interpolation, ntaps);
    const long long adv = (long long)phase + noutput * decimation;
    if (taps_per_arm) *taps_per_arm = nt;
    if (consumed) *consumed = adv / interpolation;
    if (phase_after) *phase_after = (int)(adv % interpolation);
    if (needed) *needed = rs_needed(interpolation, decimation, nt, phase, noutput);
    return MI355_OK;
}

extern "C" long long mi355_resampler_noutput_for(int interpolation, int decimation, int ntaps, int phase, long long navail_with_history)
{
    const int rc = rs_check(interpolation, decimation, ntaps);
    if (rc) return rc;
    MI355_REQUIRE(phase >= 0 && phase < interpolation, "phase outside [0, interpolation)");
    MI355_REQUIRE(navail_with_history >= 0 && navail_with_history <= (1ll << 62) / interpolation, "navail outside 0 .. 2^62 / interpolation");
    const long long nt = rs_nt(interpolation, ntaps);
    if (navail_with_history < nt) return 0;
    return ((navail_with_history - nt + 1) * interpolation - 1 - phase) / decimation + 1;
}

extern "C" int mi355_resampler_create(mi355_ctx *ctx, int interpolation, int decimation, const void *taps, int ntaps, int complex_taps,
                                      mi355_resampler **out)
{
    MI355_REQUIRE(ctx && out, "NULL argument");
    *out = nullptr;
    int rc = rs_check(interpolation, decimation, ntaps);
    if (rc) return rc;
    mi355_resampler *h = new (std::nothrow) mi355_resampler();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->L = interpolation; h->M = decimation; h->complex_taps = complex_taps ? 1 : 0;
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_resampler_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = rs_upload(h, taps, ntaps);
    }
    if (rc) { delete h; return rc; }
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_resampler_destroy(mi355_resampler *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->rev.release();
    h->d_in.release();
    h->d_out.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_resampler_set_taps(mi355_resampler *h, const void *taps, int ntaps)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return rs_upload(h, taps, ntaps);  // the phase is kept
}

extern "C" int mi355_resampler_ntaps(const mi355_resampler *h) { return h ? h->K : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_resampler_history(const mi355_resampler *h) { return h ? h->nt : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_resampler_get_taps(const mi355_resampler *h, void *taps_out, int cap)
{
    MI355_REQUIRE(h && taps_out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_resampler *>(h)->lock);
    MI355_REQUIRE(cap >= h->K, "taps_out too small");
    memcpy(taps_out, h->taps_host.data(), h->taps_host.size() * sizeof(float));
    return h->K;
}

extern "C" int mi355_resampler_get_phase(const mi355_resampler *h, int *phase)
{
    MI355_REQUIRE(h && phase, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_resampler *>(h)->lock);
    *phase = h->phase;
    return MI355_OK;
}

extern "C" int mi355_resampler_set_phase(mi355_resampler *h, int phase)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(phase >= 0 && phase < h->L, "phase outside [0, interpolation)");
    std::lock_guard<std::mutex> g(h->lock);
    h->phase = phase;
    return MI355_OK;
}

extern "C" int mi355_resampler_work_dev(mi355_resampler *h, long long noutput, const void *in_with_history, void *out, long long *consumed,
                                        void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (consumed) *consumed = 0;
    int rc = rs_args(h, noutput, in_with_history, out);
    if (rc || noutput == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_REQUIRE(!rs_overlap(in_with_history, rs_needed(h->L, h->M, h->nt, h->phase, noutput), out, noutput),
                  "clRationalResampler does not work in place: in and out overlap");
    MI355_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = mi355_pick_stream(h->ctx, stream);
    rc = rs_launch(h, noutput, h->phase, in_with_history, out, st);
    if (rc == MI355_OK) rc = h->rev.used(st);  // this table may be released behind this launch
    if (rc) return rc;
    const long long adv = (long long)h->phase + noutput * h->M;  // the phase is a kernel argument: no device state
    if (consumed) *consumed = adv / h->L;
    h->phase = (int)(adv % h->L);
    return MI355_OK;
}

extern "C" int mi355_resampler_work(mi355_resampler *h, long long noutput, const void *in_with_history, void *out, long long *consumed)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (consumed) *consumed = 0;
    int rc = rs_args(h, noutput, in_with_history, out);
    if (rc || noutput == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_REQUIRE(!rs_overlap(in_with_history, rs_needed(h->L, h->M, h->nt, h->phase, noutput), out, noutput),
                  "clRationalResampler does not work in place: in and out overlap");
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of outputs whose larger side is about kRsHostChunk items; each piece re-sends its nt - 1 samples of history
    const long long piece = mi355_piece_units(h->M > h->L ? kRsHostChunk * h->L / h->M : kRsHostChunk, noutput);
    if ((rc = h->d_in.reserve((size_t)rs_needed(h->L, h->M, h->nt, h->L - 1, piece) * 8))) return rc;
    if ((rc = h->d_out.reserve((size_t)piece * 8))) return rc;
    const char *pin = (const char *)in_with_history;
    long long used = 0;  // inputs consumed by, and the phase behind, the pieces queued so far
    int c = h->phase;
    rc = mi355_pageable_run(h->ctx, noutput, piece, [&](long long off, long long m, hipStream_t st) -> int {
        const long long need = rs_needed(h->L, h->M, h->nt, c, m), adv = (long long)c + m * h->M;
        MI355_HIP(hipMemcpyAsync(h->d_in.get(), pin + used * 8, (size_t)need * 8, hipMemcpyHostToDevice, st));
        const int lrc = rs_launch(h, m, c, h->d_in.get(), h->d_out.get(), st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + off * 8, h->d_out.get(), (size_t)m * 8, hipMemcpyDeviceToHost, st));
        used += adv / h->L;
        c = (int)(adv % h->L);
        return MI355_OK;
    });
    if (rc) return rc;
    h->phase = c;
    if (consumed) *consumed = used;
    return MI355_OK;
}
