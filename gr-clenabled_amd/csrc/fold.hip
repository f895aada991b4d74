// clFolder: exact pulsar folding of a [t][row][chan] float32 filterbank into [subint][row][bin][chan] as gfx950 HIP kernels.  The phase
// is a 64-bit integer polynomial of the absolute sample index and the sum of a (bin, channel) runs in ascending time, one binary32
// rounding per addition, so there is nothing to tolerate.  The contract is in include/mi355_clenabled.h; the reference module has
// nothing of the kind.
//
// k_fold_index  the bin-owner route's index launch, 1 / F of the data: a workgroup of 1024 threads per (sub-integration, row) computes
//               bin(T) of its Ts samples from the contract's formula, drops the flagged ones, sorts the keys (bin << 14 | t) with a
//               bitonic network in LDS -- the keys are distinct, so the order is the contract's: by bin, ascending t within a bin --
//               and leaves the per-bin lists in the scratch buffer: list[Ts] of sample offsets and start[nbin + 1]; hits are the
//               list lengths.
// k_fold_bins   the hot route: a wave owns (sub-integration, row, group of 64 V channels, a run of bins).  Lanes run along channels,
//               V = 4, 2 or 1 floats each (16-byte loads where F is a multiple of 256); per bin the wave walks its list in ascending
//               t in batches of 8 rows: 8 loads of up to 1 KiB are issued, then the 8 additions consume them in order.  The
//               accumulators never leave registers, a sample is read exactly once across the grid, there is no LDS and no atomic,
//               and a bin leaves as one whole channel run.
//               8 rows in flight per wave: the hardware guide's gather of 1,152-byte rows into registers reads at 5.5 - 5.8 TB/s
//               with 4 rows in flight per wave at 16 waves per CU (72 KiB per CU) and calls 32 KiB per CU streaming; this kernel
//               needs about 50 registers, so up to 32 waves of 8 KiB each are resident per CU, and 8 of them already hold 64 KiB.
//               Whether 4 would do is not measured.
// k_fold_gen / k_fold_gen_hits   the generic route, the route of correctness: one thread per output (or per hit count) walks the Ts
//               samples of its sub-integration, stepping the phase by its first difference (re-anchored where T wraps to 0).
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kFoMaxR = 4096, kFoMaxF = 16384, kFoMinBin = 2, kFoMaxBin = 4096, kFoMinTs = 16, kFoMaxTs = 16384;
constexpr int kFoWave = 64;
constexpr int kFoIdxThreads = 1024;
constexpr int kFoTBits = 14;                     // a key is bin << 14 | t: t < 16384, bin < 4096
constexpr uint32_t kFoPad = 0xFFFFFFFFu;         // a flagged sample, or the padding to a power of two: sorts behind every key
constexpr int kFoBatch = 8;                      // rows in flight per wave
constexpr int kFoRowsPerWave = 32;               // a wave takes a run of bins that holds about this many rows
constexpr int kFoMaxRun = 64;
constexpr long long kFoMaxCall = 1ll << 40;
constexpr size_t kFoScratchBytes = (size_t)16 << 20;  // bin-owner route: sub-integrations per chunk = what fits this, at least one
constexpr long long kFoHostBytes = 8ll << 20;         // host path: input bytes per piece unless one sub-integration needs more

template <int V> struct __attribute__((packed, aligned(4))) FV { float v[V]; };  // 4 V bytes at any 4-byte alignment

struct FoArgs {
    int R, F, nbin, Ts, V, groups, bpw, runs;
    long long nsub;
    unsigned long long T0;  // absolute index of the first sample of the launch
};

__host__ __device__ inline uint64_t fo_tri(uint64_t T) { return (T & 1u) ? T * ((T - 1) >> 1) : (T >> 1) * (T - 1); }

__host__ __device__ inline uint64_t fo_phi(uint64_t phi0, uint64_t nu, uint64_t nudot, uint64_t T) { return phi0 + nu * T + nudot * fo_tri(T); }

__host__ __device__ inline uint32_t fo_bin(uint64_t phi, uint32_t nbin) { return (uint32_t)(((phi >> 32) * (uint64_t)nbin) >> 32); }

__global__ __launch_bounds__(kFoIdxThreads) void k_fold_index(const uint64_t *__restrict__ models, const uint8_t *__restrict__ tflags,
                                                              uint32_t *__restrict__ list, uint32_t *__restrict__ start, uint32_t *__restrict__ hits,
                                                              const FoArgs a, const int P)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fo_lds[];
    uint32_t *keys = (uint32_t *)fo_lds;   // [P], P = Ts rounded up to a power of two
    uint32_t *lstart = keys + P;           // [nbin + 1]
    const int tid = threadIdx.x;
    const int R = a.R, Ts = a.Ts, nbin = a.nbin;
    const long long units = a.nsub * R;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const int r = (int)(u % R);
        const long long j = u / R;
        const uint64_t phi0 = models[3 * r], nu = models[3 * r + 1], nudot = models[3 * r + 2];
        for (int i = tid; i < P; i += kFoIdxThreads) {
            uint32_t key = kFoPad;
            if (i < Ts) {
                const long long tl = j * Ts + i;  // sample of the launch
                const uint64_t T = a.T0 + (uint64_t)tl;
                const bool flagged = tflags && tflags[(size_t)tl * R + r] != 0;
                if (!flagged) key = (fo_bin(fo_phi(phi0, nu, nudot, T), (uint32_t)nbin) << kFoTBits) | (uint32_t)i;
            }
            keys[i] = key;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int s = k >> 1; s > 0; s >>= 1) {
                for (int i = tid; i < (P >> 1); i += kFoIdxThreads) {
                    const int lo = ((i & ~(s - 1)) << 1) | (i & (s - 1)), hi = lo | s;
                    const uint32_t x = keys[lo], y = keys[hi];
                    const bool up = (lo & k) == 0;  // (k == P: every pair ascends)
                    if ((x > y) == up) {
                        keys[lo] = y;
                        keys[hi] = x;
                    }
                }
                __syncthreads();
            }
        // start[b] = the first position whose bin is >= b; start[nbin] = the number of samples that entered
        for (int i = tid; i < P; i += kFoIdxThreads) {
            const uint32_t key = keys[i];
            if (i < Ts) list[(size_t)u * Ts + i] = key & ((1u << kFoTBits) - 1u);
            const int cur = key != kFoPad ? (int)(key >> kFoTBits) : nbin;
            int prev = -1;
            if (i > 0) {
                const uint32_t kp = keys[i - 1];
                prev = kp != kFoPad ? (int)(kp >> kFoTBits) : nbin;
            }
            for (int b = prev + 1; b <= cur; b++) lstart[b] = (uint32_t)i;
            if (i == P - 1)
                for (int b = cur + 1; b <= nbin; b++) lstart[b] = (uint32_t)P;  // (P == Ts here: no padding and nothing flagged)
        }
        __syncthreads();
        for (int b = tid; b <= nbin; b += kFoIdxThreads) {
            const uint32_t s = lstart[b];
            start[(size_t)u * (nbin + 1) + b] = s;
            if (hits && b < nbin) hits[(size_t)u * nbin + b] = lstart[b + 1] - s;
        }
        __syncthreads();  // the next unit overwrites keys and lstart
    }
}

template <int V>
__global__ __launch_bounds__(256) void k_fold_bins(const float *__restrict__ in, float *__restrict__ out, const uint32_t *__restrict__ list,
                                                   const uint32_t *__restrict__ start, const FoArgs a)
{
    const int lane = threadIdx.x & (kFoWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kFoWave);
    const int R = a.R, F = a.F, nbin = a.nbin, Ts = a.Ts;
    const size_t rs = (size_t)R * F;  // floats between time samples
    const long long items = a.nsub * R * a.groups * a.runs;
    for (long long item = (long long)blockIdx.x * 4 + wave; item < items; item += (long long)gridDim.x * 4) {
        const int run = (int)(item % a.runs);
        long long q = item / a.runs;
        const int g = (int)(q % a.groups);
        q /= a.groups;
        const int r = (int)(q % R);
        const long long j = q / R;
        const size_t u = (size_t)j * R + r;
        const uint32_t *lst = list + u * Ts;
        const uint32_t *stt = start + u * (nbin + 1);
        const float *src = in + ((size_t)j * Ts * R + r) * F + g * (kFoWave * V) + V * lane;
        float *dst = out + u * nbin * F + g * (kFoWave * V) + V * lane;
        const int b1 = (run + 1) * a.bpw < nbin ? (run + 1) * a.bpw : nbin;
        for (int b = run * a.bpw; b < b1; b++) {
            const int s = (int)stt[b], e = (int)stt[b + 1];
            float acc[V];
#pragma unroll
            for (int c = 0; c < V; c++) acc[c] = 0.0f;
            int i = s;
            for (; i + kFoBatch <= e; i += kFoBatch) {  // whole batches: the 8 list entries are one scalar load, nothing is conditional
                uint32_t t[kFoBatch];
#pragma unroll
                for (int k = 0; k < kFoBatch; k++) t[k] = lst[i + k];
                FV<V> v[kFoBatch];
#pragma unroll
                for (int k = 0; k < kFoBatch; k++) v[k] = *(const FV<V> *)(src + (size_t)t[k] * rs);
#pragma unroll
                for (int k = 0; k < kFoBatch; k++) {
#pragma unroll
                    for (int c = 0; c < V; c++) acc[c] = acc[c] + v[k].v[c];
                }
            }
            if (i < e) {
                const int cnt = e - i;  // (uniform) the rows of the bin's last batch, fewer than kFoBatch
                FV<V> v[kFoBatch];
#pragma unroll
                for (int k = 0; k < kFoBatch; k++) {
#pragma unroll
                    for (int c = 0; c < V; c++) v[k].v[c] = 0.0f;
                    if (k < cnt) v[k] = *(const FV<V> *)(src + (size_t)lst[i + k] * rs);
                }
#pragma unroll
                for (int k = 0; k < kFoBatch; k++)
                    if (k < cnt) {
#pragma unroll
                        for (int c = 0; c < V; c++) acc[c] = acc[c] + v[k].v[c];
                    }
            }
            FV<V> o;
#pragma unroll
            for (int c = 0; c < V; c++) o.v[c] = acc[c];
            *(FV<V> *)(dst + (size_t)b * F) = o;
        }
    }
}

// one thread per output out[j][r][b][f] of the launch
__global__ __launch_bounds__(256) void k_fold_gen(const float *__restrict__ in, float *__restrict__ out, const uint64_t *__restrict__ models,
                                                  const uint8_t *__restrict__ tflags, const FoArgs a)
{
    const int R = a.R, F = a.F, nbin = a.nbin, Ts = a.Ts;
    const long long total = a.nsub * R * nbin * F;
    const size_t rs = (size_t)R * F;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int f = (int)(i % F);
        long long q = i / F;
        const uint32_t b = (uint32_t)(q % nbin);
        q /= nbin;
        const int r = (int)(q % R);
        const long long j = q / R;
        const uint64_t phi0 = models[3 * r], nu = models[3 * r + 1], nudot = models[3 * r + 2];
        uint64_t T = a.T0 + (uint64_t)(j * Ts);
        uint64_t phi = fo_phi(phi0, nu, nudot, T), d = nu + nudot * T;  // phi(T + 1) - phi(T) = nu + nudot T while T + 1 does not wrap
        const float *x = in + ((size_t)j * Ts * R + r) * F + f;
        const uint8_t *tf = tflags ? tflags + (size_t)j * Ts * R + r : nullptr;
        float acc = 0.0f;
        for (int t = 0; t < Ts; t++) {
            if (fo_bin(phi, (uint32_t)nbin) == b && !(tf && tf[(size_t)t * R] != 0)) acc = acc + x[(size_t)t * rs];
            T++;
            if (T == 0) { phi = phi0; d = nu; }  // the contract's phi takes the wrapped T
            else { phi += d; d += nudot; }
        }
        out[i] = acc;
    }
}

// one thread per hits[j][r][b] of the launch
__global__ __launch_bounds__(256) void k_fold_gen_hits(uint32_t *__restrict__ hits, const uint64_t *__restrict__ models, const uint8_t *__restrict__ tflags,
                                                       const FoArgs a)
{
    const int R = a.R, nbin = a.nbin, Ts = a.Ts;
    const long long total = a.nsub * R * nbin;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const uint32_t b = (uint32_t)(i % nbin);
        long long q = i / nbin;
        const int r = (int)(q % R);
        const long long j = q / R;
        const uint64_t phi0 = models[3 * r], nu = models[3 * r + 1], nudot = models[3 * r + 2];
        const uint8_t *tf = tflags ? tflags + (size_t)j * Ts * R + r : nullptr;
        uint32_t cnt = 0;
        for (int t = 0; t < Ts; t++) {
            const uint64_t T = a.T0 + (uint64_t)(j * Ts + t);
            if (fo_bin(fo_phi(phi0, nu, nudot, T), (uint32_t)nbin) == b && !(tf && tf[(size_t)t * R] != 0)) cnt++;
        }
        hits[i] = cnt;
    }
}

// everything that can be told without a device
int fo_check(int R, int F, int nbin, int Ts)
{
    MI355_REQUIRE(R >= 1 && R <= kFoMaxR, "num_rows must be 1 .. 4096");
    MI355_REQUIRE(F >= 1 && F <= kFoMaxF, "num_channels must be 1 .. 16384");
    MI355_REQUIRE(nbin >= kFoMinBin && nbin <= kFoMaxBin, "nbin must be 2 .. 4096");
    MI355_REQUIRE(Ts >= kFoMinTs && Ts <= kFoMaxTs && Ts % 16 == 0, "subint_len must be a multiple of 16 in 16 .. 16384");
    return MI355_OK;
}

int fo_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

struct mi355_fold {
    mi355_ctx *ctx = nullptr;
    int R = 0, F = 0, nbin = 0, Ts = 0;
    bool bins_ok = false, generic = false;
    long long chunk = 1;            // bin-owner route: sub-integrations per chunk
    unsigned long long T0 = 0;      // absolute index of the next sample
    std::vector<uint64_t> models;   // [R][3]
    mi355_tables dmodels;
    DevWorkspace ws;                // bin-owner route: the per-bin lists
    DevBuf d_x, d_aux;              // host path
    std::string route;
    std::mutex lock;
};

namespace {

bool fo_bins(const mi355_fold *h) { return h->bins_ok && !h->generic; }

void fo_name_route(mi355_fold *h)
{
    char buf[120];
    snprintf(buf, sizeof buf, "%s R=%d F=%d nbin=%d Ts=%d", fo_bins(h) ? "bins" : "generic", h->R, h->F, h->nbin, h->Ts);
    h->route = buf;
}

size_t fo_scratch_per_subint(const mi355_fold *h) { return (size_t)h->R * ((size_t)h->Ts + h->nbin + 1) * 4; }

// caller holds the lock and has set the device; n > 0 is a multiple of Ts; T is the absolute index of the first sample
int fo_launch(mi355_fold *h, unsigned long long T, long long n, const void *in, const void *tflags, void *out, void *hits, hipStream_t st)
{
    const int R = h->R, F = h->F, nbin = h->nbin, Ts = h->Ts;
    const long long nsub = n / Ts;
    const uint64_t *d_models = (const uint64_t *)h->dmodels.current();
    FoArgs a = {};
    a.R = R; a.F = F; a.nbin = nbin; a.Ts = Ts;
    if (!fo_bins(h)) {
        a.nsub = nsub;
        a.T0 = T;
        hipLaunchKernelGGL(k_fold_gen, dim3(mi355_grid_256(h->ctx, nsub * R * nbin * (long long)F, 32)), dim3(256), 0, st, (const float *)in, (float *)out,
                           d_models, (const uint8_t *)tflags, a);
        if (hits)
            hipLaunchKernelGGL(k_fold_gen_hits, dim3(mi355_grid_256(h->ctx, nsub * R * nbin, 32)), dim3(256), 0, st, (uint32_t *)hits, d_models,
                               (const uint8_t *)tflags, a);
        MI355_HIP(hipGetLastError());
        return h->dmodels.used(st);
    }
    a.V = F % 256 == 0 ? 4 : F % 128 == 0 ? 2 : 1;
    a.groups = F / (kFoWave * a.V);
    a.bpw = (kFoRowsPerWave * nbin + Ts - 1) / Ts;
    if (a.bpw < 1) a.bpw = 1;
    if (a.bpw > kFoMaxRun) a.bpw = kFoMaxRun;
    if (a.bpw > nbin) a.bpw = nbin;
    a.runs = (nbin + a.bpw - 1) / a.bpw;
    int rc = h->ws.acquire(h->ws.bytes(), st);  // the size of _create: nothing is allocated here
    if (rc) return rc;
    uint32_t *list = (uint32_t *)h->ws.get();
    uint32_t *start = list + (size_t)h->chunk * R * Ts;
    const int P = fo_pow2(Ts);
    const int lds = (P + nbin + 1) * 4;
    MI355_HIP(hipFuncSetAttribute((const void *)k_fold_index, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const size_t rs = (size_t)R * F;
    for (long long j0 = 0; j0 < nsub; j0 += h->chunk) {
        a.nsub = nsub - j0 < h->chunk ? nsub - j0 : h->chunk;
        a.T0 = T + (unsigned long long)(j0 * Ts);
        const float *x = (const float *)in + (size_t)j0 * Ts * rs;
        const uint8_t *tf = tflags ? (const uint8_t *)tflags + (size_t)j0 * Ts * R : nullptr;
        float *y = (float *)out + (size_t)j0 * R * nbin * F;
        uint32_t *hv = hits ? (uint32_t *)hits + (size_t)j0 * R * nbin : nullptr;
        const long long units = a.nsub * R, ucap = (long long)mi355_cus(h->ctx) * 4;
        hipLaunchKernelGGL(k_fold_index, dim3((unsigned)(units < ucap ? units : ucap)), dim3(kFoIdxThreads), (size_t)lds, st, d_models, tf, list, start,
                           hv, a, P);
        const dim3 grid(mi355_grid_256(h->ctx, units * a.groups * a.runs * kFoWave, 8));
        if (a.V == 4) hipLaunchKernelGGL(k_fold_bins<4>, grid, dim3(256), 0, st, x, y, list, start, a);
        else if (a.V == 2) hipLaunchKernelGGL(k_fold_bins<2>, grid, dim3(256), 0, st, x, y, list, start, a);
        else hipLaunchKernelGGL(k_fold_bins<1>, grid, dim3(256), 0, st, x, y, list, start, a);
    }
    MI355_HIP(hipGetLastError());
    rc = h->ws.release(st);
    if (rc) return rc;
    return h->dmodels.used(st);
}

int fo_args(const mi355_fold *h, long long n, const void *in, const void *tflags, const void *out, const void *hits)
{
    MI355_REQUIRE(n >= 0, "n is negative");
    MI355_REQUIRE(n % h->Ts == 0, "n is not a multiple of subint_len");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, "in must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, "out must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(hits) & 3u) == 0, "hits must be 4-byte aligned");
    const long long per_in = 4ll * h->R * h->F, per_out = 4ll * h->R * h->nbin * h->F, nsub = n / h->Ts;
    if (n > kFoMaxCall / per_in || nsub > kFoMaxCall / per_out) {
        mi355_set_error("clFolder: %lld samples of %lld bytes into %lld sub-integrations of %lld bytes in one call (the limit is 2^40 bytes per buffer)", n,
                        per_in, nsub, per_out);
        return MI355_ERR_UNSUPPORTED;
    }
    const void *p[4] = {in, out, tflags, hits};
    const long long pb[4] = {n * per_in, nsub * per_out, n * h->R, 4 * nsub * h->R * h->nbin};
    for (int i = 1; i < 4; i++) {
        if (!p[i]) continue;
        for (int j = 0; j < i; j++) MI355_REQUIRE(!p[j] || !mi355_overlap(p[j], pb[j], p[i], pb[i]), "two buffers overlap");
    }
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_fold_plan(int num_rows, int num_channels, int nbin, int subint_len, long long *floats_per_sample, long long *floats_per_subint,
                               long long *hits_per_subint)
{
    if (floats_per_sample) *floats_per_sample = 0;
    if (floats_per_subint) *floats_per_subint = 0;
    if (hits_per_subint) *hits_per_subint = 0;
    const int rc = fo_check(num_rows, num_channels, nbin, subint_len);
    if (rc) return rc;
    if (floats_per_sample) *floats_per_sample = (long long)num_rows * num_channels;
    if (floats_per_subint) *floats_per_subint = (long long)num_rows * nbin * num_channels;
    if (hits_per_subint) *hits_per_subint = (long long)num_rows * nbin;
    return MI355_OK;
}

extern "C" int mi355_fold_create(mi355_ctx *ctx, int num_rows, int num_channels, int nbin, int subint_len, const uint64_t *models, mi355_fold **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    int rc = fo_check(num_rows, num_channels, nbin, subint_len);
    if (rc) return rc;
    MI355_REQUIRE(models != nullptr, "models is NULL");
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_fold *h = new (std::nothrow) mi355_fold();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->R = num_rows; h->F = num_channels; h->nbin = nbin; h->Ts = subint_len;
    h->bins_ok = h->F % kFoWave == 0;
    h->models.assign(models, models + 3 * (size_t)h->R);
    const size_t per = fo_scratch_per_subint(h);
    h->chunk = (long long)(kFoScratchBytes / per);
    if (h->chunk < 1) h->chunk = 1;
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_fold_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = h->dmodels.publish(ctx, h->models.data(), h->models.size() * 8, "mi355_fold: models");
        if (rc == MI355_OK && h->bins_ok) rc = h->ws.acquire((size_t)h->chunk * per, ctx->stream[0]);
    }
    if (rc) { mi355_fold_destroy(h); return rc; }
    fo_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clFolder: %d rows, %d channels, %d bins, sub-integrations of %d: %s", h->R, h->F, h->nbin, h->Ts, h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_fold_destroy(mi355_fold *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)h->ws.wait();
    h->ws.destroy();
    h->dmodels.release();
    h->d_x.release();
    h->d_aux.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_fold_set_models(mi355_fold *h, const uint64_t *models)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(models != nullptr, "models is NULL");
    std::vector<uint64_t> img(models, models + 3 * (size_t)h->R);
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const int rc = h->dmodels.publish(h->ctx, img.data(), img.size() * 8, "mi355_fold: models");  // on failure the version in use stays
    if (rc) return rc;
    h->models.swap(img);
    return MI355_OK;
}

extern "C" int mi355_fold_get_models(const mi355_fold *h, uint64_t *out, long long cap_words)
{
    MI355_REQUIRE(h && out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_fold *>(h)->lock);
    MI355_REQUIRE(cap_words >= (long long)h->models.size(), "out too small");
    memcpy(out, h->models.data(), h->models.size() * 8);
    return MI355_OK;
}

extern "C" int mi355_fold_sample(const mi355_fold *h, unsigned long long *T)
{
    MI355_REQUIRE(h && T, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_fold *>(h)->lock);
    *T = h->T0;
    return MI355_OK;
}

extern "C" int mi355_fold_set_sample(mi355_fold *h, unsigned long long T)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->T0 = T;
    return MI355_OK;
}

extern "C" int mi355_fold_skip(mi355_fold *h, long long n)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(n >= 0, "n is negative");
    std::lock_guard<std::mutex> g(h->lock);
    h->T0 += (unsigned long long)n;
    return MI355_OK;
}

extern "C" long long mi355_fold_subint_len(const mi355_fold *h) { return h ? h->Ts : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_fold_set_generic(mi355_fold *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    fo_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_fold_route(const mi355_fold *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_fold_work_dev(mi355_fold *h, long long n, const void *in, const void *tflags, void *out, void *hits, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = fo_args(h, n, in, tflags, out, hits);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const int lrc = fo_launch(h, h->T0, n, in, tflags, out, hits, mi355_pick_stream(h->ctx, stream));
    if (lrc == MI355_OK) h->T0 += (unsigned long long)n;
    return lrc;
}

extern "C" int mi355_fold_work(mi355_fold *h, long long n, const void *in, const void *tflags, void *out, void *hits)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = fo_args(h, n, in, tflags, out, hits);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole sub-integrations; the archive, the hits and the flags of a piece lie behind one another in d_aux
    const long long R = h->R, F = h->F, nbin = h->nbin, Ts = h->Ts, nsub = n / Ts;
    const long long in_bytes = 4 * Ts * R * F, out_bytes = 4 * R * nbin * F, hit_bytes = 4 * R * nbin, tf_bytes = Ts * R;
    const long long piece = mi355_piece_units(kFoHostBytes / in_bytes, nsub);
    if ((rc = h->d_x.reserve((size_t)(piece * in_bytes)))) return rc;
    if ((rc = h->d_aux.reserve((size_t)(piece * (out_bytes + hit_bytes + tf_bytes))))) return rc;
    char *d_out = (char *)h->d_aux.get(), *d_hit = d_out + piece * out_bytes, *d_tf = d_hit + piece * hit_bytes;
    const unsigned long long T0 = h->T0;
    rc = mi355_pageable_run(h->ctx, nsub, piece, [&](long long j0, long long nj, hipStream_t st) -> int {
        MI355_HIP(hipMemcpyAsync(h->d_x.get(), (const char *)in + (size_t)(j0 * in_bytes), (size_t)(nj * in_bytes), hipMemcpyHostToDevice, st));
        if (tflags) MI355_HIP(hipMemcpyAsync(d_tf, (const char *)tflags + (size_t)(j0 * tf_bytes), (size_t)(nj * tf_bytes), hipMemcpyHostToDevice, st));
        const int lrc = fo_launch(h, T0 + (unsigned long long)(j0 * Ts), nj * Ts, h->d_x.get(), tflags ? d_tf : nullptr, d_out, hits ? d_hit : nullptr, st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + (size_t)(j0 * out_bytes), d_out, (size_t)(nj * out_bytes), hipMemcpyDeviceToHost, st));
        if (hits) MI355_HIP(hipMemcpyAsync((char *)hits + (size_t)(j0 * hit_bytes), d_hit, (size_t)(nj * hit_bytes), hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
    if (rc == MI355_OK) h->T0 = T0 + (unsigned long long)n;
    return rc;
}

// host only: the three words of a row's phase model, computed in long double
extern "C" int mi355_fold_model(double period_s, double pdot, double tsamp_s, double phase0_turns, uint64_t out[3])
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    MI355_REQUIRE(std::isfinite(period_s) && std::isfinite(pdot) && std::isfinite(tsamp_s) && std::isfinite(phase0_turns), "non-finite argument");
    MI355_REQUIRE(period_s > 0.0 && tsamp_s > 0.0, "period and tsamp must be positive");
    const long double two64 = 18446744073709551616.0L;
    const long double q = (long double)tsamp_s / (long double)period_s;  // turns per sample
    const long double nd = -(long double)pdot * q * q;                   // turns per sample^2: fdot tsamp^2 with fdot = -pdot / period^2
    MI355_REQUIRE(std::isfinite(q) && std::isfinite(nd) && fabsl(nd) < 0.5L, "the model does not fit: tsamp / period overflows or |nudot| >= 1/2 turn per sample^2");
    // phi(T) = f0 t + fdot t^2 / 2 at t = T tsamp is nu T + nudot T (T - 1) / 2 with nu = q + nudot / 2
    auto frac_word = [&](long double x) -> uint64_t {
        long double v = rintl((x - floorl(x)) * two64);
        if (v >= two64) v -= two64;
        return (uint64_t)v;
    };
    const long double ndw = rintl(nd * two64);  // |ndw| <= 2^63
    out[0] = frac_word((long double)phase0_turns);
    out[1] = frac_word(q + nd * 0.5L);
    out[2] = ndw >= 9223372036854775808.0L ? (uint64_t)INT64_MAX : ndw <= -9223372036854775808.0L ? (uint64_t)INT64_MIN : (uint64_t)(int64_t)ndw;
    return MI355_OK;
}

// host only: bin(T) of T = T0 .. T0 + n - 1, bit for bit as the device computes it
extern "C" int mi355_fold_bins(const uint64_t model[3], uint64_t T0, long long n, int nbin, int32_t *bins)
{
    MI355_REQUIRE(model != nullptr, "NULL argument");
    MI355_REQUIRE(n >= 0, "n is negative");
    MI355_REQUIRE(nbin >= kFoMinBin && nbin <= kFoMaxBin, "nbin must be 2 .. 4096");
    MI355_REQUIRE(n == 0 || bins != nullptr, "NULL argument");
    for (long long i = 0; i < n; i++) bins[i] = (int32_t)fo_bin(fo_phi(model[0], model[1], model[2], T0 + (uint64_t)i), (uint32_t)nbin);
    return MI355_OK;
}
