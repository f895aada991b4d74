// clDedisperser: exact incoherent dedispersion of a [t][row][chan] float32 filterbank over D dispersion-measure trials as gfx950 HIP
// kernels.  The contract is in include/mi355_clenabled.h; the reference module has no dedisperser.
//
//     y(r, d, t) = (((+0.0f + x[t + delay[d][0]][r][0]) + x[t + delay[d][1]][r][1]) + ...)       every f with delay[d][f] == -1 skipped
//
// binary32 additions in ascending channel order, one rounding each: the channel sum of one output is never split across threads, so
// the bits are a function of the inputs alone (no float atomics, no partial sums).
//
// k_dd_tiled  the hot route.  A workgroup of two waves owns (row, tile of kDdDT = 16 trials, tile of kDdTT = 256 output samples) and walks
//             the channels in blocks of kDdFB = 8.  Per block it loads -- 8 lanes along f, 16 along time: runs of 32 bytes -- only the
//             time window its trials need, [t0 + min delay, t0 + 256 + max delay) from the host-side min/max table of the (trial tile,
//             channel block), and stores it to LDS transposed, lds[f][time], pitch 392 (8 mod 32: the 64 lanes of a transposing store
//             fall on 32 banks twice, which a 4-byte store does for free).  Wave w owns trials 8 w .. 8 w + 7 of the tile and a lane the
//             four outputs t0 + lane + 64 k, so lds[f][t + delay] is 64 consecutive addresses per read and one address computation
//             serves four reads (immediate offsets 256 k bytes).  The delays of a (trial tile, channel) lie together in a re-ordered
//             copy of the table, a wave's 8 arrive as ONE 32-byte scalar load; a (wave, channel) without a -1 is one straight-line
//             block with its reads in flight together, skipping a -1 is a scalar branch.  The 32 accumulators stay in registers across
//             all channel blocks; the next block's global loads (24 registers) are issued before the current block is summed.
//             The route needs max - min <= kDdSpread = 128 in every (trial tile, channel block), and a window of less than 2^32 bytes
//             (R F <= 2796202: 32-bit lane offsets from a uniform base); anything else runs generic.
// k_dd_gen    the generic route: one thread per output, lanes along time, delays and samples through the caches.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

constexpr int kDdMaxR = 4096, kDdMaxF = 16384, kDdMaxD = 4096, kDdMaxH = 1 << 20;
constexpr int kDdWave = 64;
constexpr int kDdWaves = 2, kDdThreads = kDdWave * kDdWaves;
constexpr int kDdK = 4;                          // outputs per lane
constexpr int kDdTT = kDdWave * kDdK;            // outputs per workgroup
constexpr int kDdDW = 8;                         // trials per wave
constexpr int kDdDT = kDdDW * kDdWaves;          // trials per workgroup
constexpr int kDdFB = 8;                         // channels per block
constexpr int kDdSpread = 128;                   // largest max - min delay of a (trial tile, channel block) the LDS plan holds
constexpr int kDdRows = kDdTT + kDdSpread;       // time samples of a block's window at most
constexpr int kDdPitch = kDdRows + 8;            // = 8 (mod 32)
constexpr int kDdNPF = kDdRows / (kDdThreads / kDdFB);  // window samples a lane carries from global memory to LDS per block
constexpr long long kDdMaxCall = 1ll << 40;
constexpr long long kDdMaxTable = 1ll << 30;
static_assert(kDdPitch % 32 == 8 && kDdThreads % kDdFB == 0 && kDdRows % (kDdThreads / kDdFB) == 0, "LDS plan");

struct DdArgs {
    int R, F, D, ntd, nfb;
    long long n, ntot;    // outputs of the call, input samples of the call = n + H
    long long pitch;      // floats between the time series of TRIAL_MAJOR
    long long units;      // workgroup units: trial tiles x rows x time tiles, trial tile fastest (neighbours share their input in L2)
};

// tabT: [trial tile][f][16 trials], the last tile filled up with copies of trial D - 1 (summed, never stored)
// mmt:  [trial tile][channel block] {min, max} over the entries that are not -1 ({0, 0} if there is none)
// (the pointers are __restrict__ kernel arguments so that the uniform table reads are scalar loads)
template <int ORDER>
__global__ __launch_bounds__(kDdThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_dd_tiled(const float *__restrict__ in, float *__restrict__ out,
                                                                                               const v8i *__restrict__ tabT_all,
                                                                                               const int2 *__restrict__ mm_all, const DdArgs a)
{
    __shared__ __attribute__((aligned(16))) float lds[kDdFB * kDdPitch];
    const int tid = threadIdx.x, lane = tid & (kDdWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kDdWave);  // this wave's 8 trials of the tile
    const int lf = tid & (kDdFB - 1), lt = tid / kDdFB;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int dtile = (int)(u % a.ntd);
        const long long q = u / a.ntd;
        const int r = (int)(q % a.R);
        const long long t0 = (q / a.R) * kDdTT;
        const int2 *mm = mm_all + (size_t)dtile * a.nfb;
        const v8i *tabT = tabT_all + (size_t)dtile * a.F * kDdWaves + wave;
        float acc[kDdDW][kDdK];
#pragma unroll
        for (int j = 0; j < kDdDW; j++)
#pragma unroll
            for (int k = 0; k < kDdK; k++) acc[j][k] = 0.0f;
        float pf[kDdNPF];
        // the window of block b: samples tb .. tb + W - 1 of channels b 8 .. b 8 + 7; nothing outside [0, n + H) x [0, F) is read
        // and no lane branches: a sample past the call's input or a channel past F is replaced by the nearest one inside, which only
        // outputs t >= n (never stored) and channels >= F (never summed) would see
        auto load = [&](int b) {
            const int2 m = mm[b];
            const int W = kDdTT + m.y - m.x;
            const long long tb = t0 + m.x;
            // a uniform base and 32-bit lane byte offsets (the route is only taken when 4 R F kDdRows < 2^32)
            const char *src = (const char *)(in + ((size_t)tb * a.R + r) * a.F + b * kDdFB);
            const long long left = a.ntot - tb;  // samples from tb to the end of the call's input, >= 1
            const unsigned rows = left < W ? (unsigned)left : (unsigned)W;
            const unsigned rs4 = 4u * (unsigned)a.R * (unsigned)a.F;
            const unsigned nfb = (unsigned)(a.F - b * kDdFB);  // channels from this block's first to the last, >= 1
            const unsigned lf4 = 4u * ((unsigned)lf < nfb ? (unsigned)lf : nfb - 1);
            const unsigned last = (rows - 1) * rs4 + lf4;
            const unsigned first = (unsigned)lt * rs4 + lf4;
#pragma unroll
            for (int i = 0; i < kDdNPF; i++) {
                unsigned off = first + (unsigned)(i * (kDdThreads / kDdFB)) * rs4;
                off = off < last ? off : last;
                pf[i] = *(const float *)(src + off);
            }
        };
        load(0);
        for (int b = 0; b < a.nfb; b++) {
            __syncthreads();  // the previous block has been summed
#pragma unroll
            for (int i = 0; i < kDdNPF; i++) lds[lf * kDdPitch + i * (kDdThreads / kDdFB) + lt] = pf[i];
            __syncthreads();
            const int mn = mm[b].x;
            if (b + 1 < a.nfb) load(b + 1);
            const int f0 = b * kDdFB;
            const int nf = a.F - f0 < kDdFB ? a.F - f0 : kDdFB;
            for (int fl = 0; fl < nf; fl++) {
                const v8i dv = tabT[(f0 + fl) * kDdWaves];
                const float *row = lds + fl * kDdPitch + lane - mn;
                int any = 0;
#pragma unroll
                for (int j = 0; j < kDdDW; j++) any |= dv[j];
                if (any >= 0) {  // (uniform) no -1 among the 8: one block of straight-line code, the reads in flight together
#pragma unroll
                    for (int j = 0; j < kDdDW; j++)
#pragma unroll
                        for (int k = 0; k < kDdK; k++) acc[j][k] = acc[j][k] + row[dv[j] + k * kDdWave];
                } else {
#pragma unroll
                    for (int j = 0; j < kDdDW; j++) {
                        const int dl = dv[j];
                        if (dl >= 0) {  // (uniform)
#pragma unroll
                            for (int k = 0; k < kDdK; k++) acc[j][k] = acc[j][k] + row[dl + k * kDdWave];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kDdK; k++) {
            const long long t = t0 + lane + k * kDdWave;
            if (t < a.n) {
#pragma unroll
                for (int j = 0; j < kDdDW; j++) {
                    const int d = dtile * kDdDT + wave * kDdDW + j;
                    if (d < a.D) {
                        if (ORDER == MI355_DEDISP_TRIAL_MAJOR) out[((size_t)r * a.D + d) * (size_t)a.pitch + (size_t)t] = acc[j][k];
                        else out[((size_t)t * a.R + r) * a.D + d] = acc[j][k];
                    }
                }
            }
        }
    }
}

// generic route: one thread per output, lanes along time
template <int ORDER>
__global__ __launch_bounds__(256) void k_dd_gen(const float *__restrict__ in, const int *__restrict__ tab, float *__restrict__ out, int R, int F, int D,
                                                long long n, long long pitch)
{
    const long long total = (long long)R * D * n;
    const size_t rowstride = (size_t)R * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i % n, rd = i / n;
        const int d = (int)(rd % D), r = (int)(rd / D);
        const int *dl = tab + (size_t)d * F;
        const float *x = in + (size_t)r * F;
        float acc = 0.0f;
        for (int f = 0; f < F; f++) {
            const int dd = dl[f];
            if (dd >= 0) acc = acc + x[(size_t)(t + dd) * rowstride + f];
        }
        if (ORDER == MI355_DEDISP_TRIAL_MAJOR) out[(size_t)rd * (size_t)pitch + (size_t)t] = acc;
        else out[((size_t)t * R + r) * D + d] = acc;
    }
}

// everything that can be told without a device
int dd_check(int R, int F, int D, int H, int order)
{
    MI355_REQUIRE(R >= 1 && R <= kDdMaxR, "num_rows must be 1 .. 4096");
    MI355_REQUIRE(F >= 1 && F <= kDdMaxF, "num_channels must be 1 .. 16384");
    MI355_REQUIRE(D >= 1 && D <= kDdMaxD, "num_trials must be 1 .. 4096");
    MI355_REQUIRE(H >= 0 && H <= kDdMaxH, "max_delay must be 0 .. 2^20");
    MI355_REQUIRE(order == MI355_DEDISP_TRIAL_MAJOR || order == MI355_DEDISP_TIME_MAJOR, "order must be TRIAL_MAJOR (0) or TIME_MAJOR (1)");
    if (4ll * D * F > kDdMaxTable) {
        mi355_set_error("clDedisperser: a delay table of 4 x %d x %d bytes is above 1 GiB", D, F);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

int dd_check_table(const int *tab, size_t n, int H)
{
    for (size_t i = 0; i < n; i++) MI355_REQUIRE(tab[i] >= -1 && tab[i] <= H, "a delay outside -1 .. max_delay");
    return MI355_OK;
}

}  // namespace

struct mi355_dedisp {
    mi355_ctx *ctx = nullptr;
    int R = 0, F = 0, D = 0, H = 0, order = 0;
    int ntd = 0, nfb = 0;
    size_t raw_bytes = 0, raw_pad = 0, tabT_bytes = 0, mm_bytes = 0;
    bool generic = false;
    bool fits32 = false;   // a block's window spans less than 2^32 bytes: the tiled kernel's lane offsets are 32-bit
    std::vector<int> tab;  // the caller's layout
    mi355_tables dtab;     // [the caller's table | re-ordered table | min/max table]
    bool tiled = false;    // the LDS plan holds every window of the table in use
    HostPipe pipe;
    std::string route;
    std::mutex lock;
};

namespace {

void dd_name_route(mi355_dedisp *h)
{
    char buf[160];
    if (h->tiled && h->fits32 && !h->generic)
        snprintf(buf, sizeof buf, "tiled R=%d F=%d D=%d fb=%d dt=%d tt=%d", h->R, h->F, h->D, kDdFB, kDdDT, kDdTT);
    else snprintf(buf, sizeof buf, "generic R=%d F=%d D=%d", h->R, h->F, h->D);
    h->route = buf;
}

// a new version from `tab`; caller holds the lock (or is create) and has set the device.  On failure the version in use is unchanged.
int dd_upload(mi355_dedisp *h, const int *tab)
{
    const int F = h->F, D = h->D;
    std::vector<char> img(h->raw_pad + h->tabT_bytes + h->mm_bytes, 0);
    memcpy(img.data(), tab, h->raw_bytes);
    int *tabT = (int *)(img.data() + h->raw_pad);
    int *mm = (int *)(img.data() + h->raw_pad + h->tabT_bytes);
    bool tiled = true;
    for (int dt = 0; dt < h->ntd; dt++) {
        for (int f = 0; f < F; f++)
            for (int j = 0; j < kDdDT; j++) {
                const int d = dt * kDdDT + j;
                tabT[((size_t)dt * F + f) * kDdDT + j] = tab[(size_t)(d < D ? d : D - 1) * F + f];
            }
        for (int b = 0; b < h->nfb; b++) {
            int lo = INT32_MAX, hi = -1;
            for (int f = b * kDdFB; f < F && f < (b + 1) * kDdFB; f++)
                for (int j = 0; j < kDdDT; j++) {
                    const int v = tabT[((size_t)dt * F + f) * kDdDT + j];
                    if (v < 0) continue;
                    if (v < lo) lo = v;
                    if (v > hi) hi = v;
                }
            if (hi < 0) lo = hi = 0;
            mm[((size_t)dt * h->nfb + b) * 2] = lo;
            mm[((size_t)dt * h->nfb + b) * 2 + 1] = hi;
            if (hi - lo > kDdSpread) tiled = false;
        }
    }
    const int rc = h->dtab.publish(h->ctx, img.data(), img.size(), "mi355_dedisp: table");
    if (rc == MI355_OK) h->tiled = tiled;
    return rc;
}

// caller holds the lock and has set the device
int dd_launch(mi355_dedisp *h, long long n, const void *in, void *out, long long pitch, hipStream_t st)
{
    const int cus = mi355_cus(h->ctx);
    const char *d_tab = (const char *)h->dtab.current();
    const int *d_raw = (const int *)d_tab;
    if (h->tiled && h->fits32 && !h->generic) {
        DdArgs a = {};
        const v8i *tabT = (const v8i *)(d_tab + h->raw_pad);
        const int2 *mm = (const int2 *)(d_tab + h->raw_pad + h->tabT_bytes);
        a.R = h->R; a.F = h->F; a.D = h->D; a.ntd = h->ntd; a.nfb = h->nfb;
        a.n = n; a.ntot = n + h->H; a.pitch = pitch;
        const long long ntt = (n + kDdTT - 1) / kDdTT;
        a.units = ntt * h->R * h->ntd;
        const long long cap = (long long)cus * 48;  // up to 12 resident workgroups per CU (12.25 KiB of LDS each), four rounds
        const dim3 grid((unsigned)(a.units < cap ? a.units : cap));
        if (h->order == MI355_DEDISP_TRIAL_MAJOR) hipLaunchKernelGGL(k_dd_tiled<MI355_DEDISP_TRIAL_MAJOR>, grid, dim3(kDdThreads), 0, st, (const float *)in, (float *)out, tabT, mm, a);
        else hipLaunchKernelGGL(k_dd_tiled<MI355_DEDISP_TIME_MAJOR>, grid, dim3(kDdThreads), 0, st, (const float *)in, (float *)out, tabT, mm, a);
    } else {
        const long long total = n * h->R * h->D;
        const long long blocks = (total + 255) / 256, cap = (long long)cus * 32;
        const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
        if (h->order == MI355_DEDISP_TRIAL_MAJOR)
            hipLaunchKernelGGL(k_dd_gen<MI355_DEDISP_TRIAL_MAJOR>, grid, dim3(256), 0, st, (const float *)in, d_raw, (float *)out, h->R, h->F, h->D, n, pitch);
        else
            hipLaunchKernelGGL(k_dd_gen<MI355_DEDISP_TIME_MAJOR>, grid, dim3(256), 0, st, (const float *)in, d_raw, (float *)out, h->R, h->F, h->D, n, pitch);
    }
    MI355_HIP(hipGetLastError());
    return h->dtab.used(st);  // this version may be released behind this launch
}

// floats from the first to one past the last that a call for n outputs may write
long long dd_out_extent(const mi355_dedisp *h, long long n, long long pitch)
{
    if (h->order == MI355_DEDISP_TIME_MAJOR) return n * h->R * h->D;
    return ((long long)h->R * h->D - 1) * pitch + n;
}

int dd_args(const mi355_dedisp *h, long long n, const void *in, const void *out, long long pitch)
{
    MI355_REQUIRE(n >= 0, "n is negative");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, "in must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, "out must be 4-byte aligned");
    if (h->order == MI355_DEDISP_TIME_MAJOR) MI355_REQUIRE(pitch == 0, "out_pitch must be 0 in TIME_MAJOR order");
    else MI355_REQUIRE(pitch >= n, "out_pitch is below n");
    const long long in_per = 4ll * h->R * h->F, rd = (long long)h->R * h->D;
    const long long span = h->order == MI355_DEDISP_TIME_MAJOR ? n : pitch;  // floats per (row, trial) of the output's extent, at most
    if (n > kDdMaxCall / in_per - h->H || span > kDdMaxCall / (4 * rd)) {
        mi355_set_error("clDedisperser: %lld outputs of %lld input and %lld output bytes in one call (the limit is 2^40 bytes per buffer)", n, in_per,
                        4 * rd);
        return MI355_ERR_UNSUPPORTED;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    MI355_REQUIRE(!(a < b + (uintptr_t)(4 * dd_out_extent(h, n, pitch)) && b < a + (uintptr_t)((n + h->H) * in_per)),
                  "clDedisperser does not work in place: in and out overlap");
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_dedisp_plan(int num_rows, int num_channels, int num_trials, int max_delay, int order, long long *in_floats_per_sample,
                                 long long *history, long long *out_floats_per_sample)
{
    if (in_floats_per_sample) *in_floats_per_sample = 0;
    if (history) *history = 0;
    if (out_floats_per_sample) *out_floats_per_sample = 0;
    const int rc = dd_check(num_rows, num_channels, num_trials, max_delay, order);
    if (rc) return rc;
    if (in_floats_per_sample) *in_floats_per_sample = (long long)num_rows * num_channels;
    if (history) *history = max_delay;
    if (out_floats_per_sample) *out_floats_per_sample = (long long)num_rows * num_trials;
    return MI355_OK;
}

extern "C" int mi355_dedisp_create(mi355_ctx *ctx, int num_rows, int num_channels, int num_trials, int max_delay, int order, const int32_t *delays,
                                   mi355_dedisp **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    int rc = dd_check(num_rows, num_channels, num_trials, max_delay, order);
    if (rc) return rc;
    const size_t nt = (size_t)num_trials * num_channels;
    if (delays) {
        rc = dd_check_table(delays, nt, max_delay);
        if (rc) return rc;
    }
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_dedisp *h = new (std::nothrow) mi355_dedisp();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->R = num_rows; h->F = num_channels; h->D = num_trials; h->H = max_delay; h->order = order;
    h->ntd = (h->D + kDdDT - 1) / kDdDT;
    h->nfb = (h->F + kDdFB - 1) / kDdFB;
    h->fits32 = 4ll * h->R * h->F * kDdRows < (1ll << 32);
    h->raw_bytes = nt * 4;
    h->raw_pad = (h->raw_bytes + 255) & ~(size_t)255;
    h->tabT_bytes = (size_t)h->ntd * h->F * kDdDT * 4;
    h->mm_bytes = (size_t)h->ntd * h->nfb * 8;
    if (delays) h->tab.assign(delays, delays + nt);
    else h->tab.assign(nt, 0);
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_dedisp_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = dd_upload(h, h->tab.data());
        if (rc == MI355_OK) rc = h->pipe.init(ctx);
    }
    if (rc) { mi355_dedisp_destroy(h); return rc; }
    dd_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clDedisperser: %d rows, %d channels, %d trials, max delay %d, %s: %s", h->R, h->F, h->D, h->H,
              order == MI355_DEDISP_TIME_MAJOR ? "time major" : "trial major", h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_dedisp_destroy(mi355_dedisp *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->dtab.release();
    h->pipe.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_dedisp_set_delays(mi355_dedisp *h, const int32_t *delays)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(delays != nullptr, "delays is NULL");
    const size_t nt = (size_t)h->D * h->F;
    const int rc = dd_check_table(delays, nt, h->H);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const int rc2 = dd_upload(h, delays);  // on failure the version in use and its host copy stay
    if (rc2) return rc2;
    h->tab.assign(delays, delays + nt);
    dd_name_route(h);
    return MI355_OK;
}

extern "C" int mi355_dedisp_get_delays(const mi355_dedisp *h, int32_t *out, long long cap_entries)
{
    MI355_REQUIRE(h && out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_dedisp *>(h)->lock);
    MI355_REQUIRE(cap_entries >= (long long)h->tab.size(), "out too small");
    memcpy(out, h->tab.data(), h->tab.size() * 4);
    return MI355_OK;
}

extern "C" long long mi355_dedisp_history(const mi355_dedisp *h) { return h ? h->H : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_dedisp_set_generic(mi355_dedisp *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    dd_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_dedisp_route(const mi355_dedisp *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_dedisp_work_dev(mi355_dedisp *h, long long n, const void *in, void *out, long long out_pitch, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = dd_args(h, n, in, out, out_pitch);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return dd_launch(h, n, in, out, out_pitch, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_dedisp_work(mi355_dedisp *h, long long n, const void *in, void *out, long long out_pitch)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = dd_args(h, n, in, out, out_pitch);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole output samples, each staged with its H samples of look-ahead; one staging slot: the pieces run one after the other
    const size_t per_in = (size_t)4 * h->R * h->F, per_out = (size_t)4 * h->R * h->D, rd = (size_t)h->R * h->D;
    const size_t bigger = per_in > per_out ? per_in : per_out;
    size_t piece = mi355_chunk_bytes((size_t)n * bigger, h->ctx) / bigger;
    if (piece < 1) piece = 1;
    if (piece > (size_t)n) piece = (size_t)n;
    const size_t in_cap = (piece + h->H) * per_in;
    rc = h->pipe.ensure(1, &in_cap, piece * per_out, 1);
    if (rc) return rc;
    const HostPipe::Plan plan{1, true, false};  // one slot, stream[0], never direct
    const bool time_major = h->order == MI355_DEDISP_TIME_MAJOR;
    auto samples = [&](size_t ci) { return HostPipe::part((size_t)n, piece, ci); };
    return h->pipe.run(
        ((size_t)n + piece - 1) / piece, plan,
        [&](size_t ci) { return HostPipe::Chunk{{(const char *)in + ci * piece * per_in}, {(samples(ci) + h->H) * per_in}, nullptr, samples(ci) * per_out}; },
        [&](size_t ci, void *const *d_in, void *d_out, hipStream_t st) {
            return dd_launch(h, (long long)samples(ci), d_in[0], d_out, time_major ? 0 : (long long)samples(ci), st);
        },
        [&](size_t ci, const void *h_out) {
            const size_t off = ci * piece, m = samples(ci);
            if (time_major) mi355_copy((char *)out + off * per_out, h_out, m * per_out);
            else  // channel-major: row i of the piece goes to its place in the caller's row
                for (size_t i = 0; i < rd; i++) memcpy((float *)out + i * (size_t)out_pitch + off, (const float *)h_out + i * m, m * 4);
        });
}

// host only: delay[d][f] = llrint(4.148808e3 dm[d] (nu_f^-2 - nu_ref^-2) / tsamp), nu^-2 = 1 / (nu nu), every operation rounded on its own
extern "C" int mi355_dedisp_delays(double f0_mhz, double df_mhz, int num_channels, double tsamp_s, const double *dm, int num_trials, int32_t *out,
                                   int *max_delay)
{
#pragma clang fp contract(off)
    if (max_delay) *max_delay = 0;
    MI355_REQUIRE(dm && out, "NULL argument");
    MI355_REQUIRE(num_channels >= 1 && num_channels <= kDdMaxF, "num_channels must be 1 .. 16384");
    MI355_REQUIRE(num_trials >= 1 && num_trials <= kDdMaxD, "num_trials must be 1 .. 4096");
    MI355_REQUIRE(std::isfinite(tsamp_s) && tsamp_s > 0.0, "tsamp_s must be positive");
    std::vector<double> inv2((size_t)num_channels);
    double nu_ref = 0.0;
    for (int f = 0; f < num_channels; f++) {
        const double step = (double)f * df_mhz;
        const double nu = f0_mhz + step;
        MI355_REQUIRE(std::isfinite(nu) && nu > 0.0, "a channel frequency that is not positive");
        if (nu > nu_ref) nu_ref = nu;
        const double sq = nu * nu;
        inv2[f] = 1.0 / sq;
    }
    const double sqr = nu_ref * nu_ref;
    const double inv_ref = 1.0 / sqr;
    for (int d = 0; d < num_trials; d++) MI355_REQUIRE(std::isfinite(dm[d]) && dm[d] >= 0.0, "a dispersion measure that is negative or not finite");
    long long top = 0;
    for (int d = 0; d < num_trials; d++) {
        const double k = 4.148808e3 * dm[d];
        for (int f = 0; f < num_channels; f++) {
            const double diff = inv2[f] - inv_ref;
            const double prod = k * diff;
            const double v = prod / tsamp_s;
            MI355_REQUIRE(v <= (double)kDdMaxH + 0.5, "a delay above 2^20 samples");
            const long long q = llrint(v);
            MI355_REQUIRE(q >= 0 && q <= kDdMaxH, "a delay above 2^20 samples");
            out[(size_t)d * num_channels + f] = (int32_t)q;
            if (q > top) top = q;
        }
    }
    if (max_delay) *max_delay = (int)top;
    return MI355_OK;
}
