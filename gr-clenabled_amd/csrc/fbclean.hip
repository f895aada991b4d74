// clFilterbankCleaner: exact RFI excision of a [t][row][chan] float32 filterbank ahead of clDedisperser as gfx950 HIP kernels: per
// (block of Tb samples, row, channel) float64 statistics in a pinned order, a spectral-kurtosis / variance / static-mask channel flag,
// normalisation to zero mean and unit variance, and the zero-DM filter with a broadband time-sample flag.  The contract is in
// include/mi355_clenabled.h; the reference module has nothing of the kind.
//
// k_fb_slab   the hot route: ONE launch, a workgroup of 16 waves owns one (block, row) slab of Tb x F floats; nothing of steps 1 - 4
//             reaches outside a slab, so there is no grid-wide step.
//             Phase A, per group of 256 channels: wave s is segment s of the block, a lane owns 4 adjacent channels (16-byte loads:
//             a wave reads the whole 1 KiB run of a time sample, R F 4 bytes apart), a1 / a2 in 16 float64 registers over the
//             segment's Tb/16 samples in ascending t.  The 16 segment sums of the group meet in LDS (64 KiB); after a barrier
//             thread c < 256 adds the 16 of channel c in the contract's adjacent-pair tree, runs step 2 once and leaves m32, is32
//             and good in LDS (9 F bytes), writes cflags / stats and counts the good channels (integer LDS atomic).
//             Phase B, after the last group's barrier: wave w takes the time samples w, w + 16, ... of the block; its lanes read the
//             row with the same 16-byte pattern, normalise into registers (4 F / 256 floats per lane), add their float64 partial
//             in ascending f -- exactly p_lane of the contract -- and reduce it with an xor butterfly across the 64 lanes (the
//             adjacent-pair tree: IEEE addition commutes), then subtract and store 16 bytes per lane; lane 0 writes the tflag.
//             The slab is read twice and written once; a row is read whole before it is written, so out == in is safe.
//             Domain: F a multiple of 256 in 256 .. 4096, every Tb.
// k_fb_stat / k_fb_zdm / k_fb_apply   the generic route, the route of correctness: one thread per (block, row, channel) walks the
//             contract's order, one thread per (t, row) does the zero-DM sum, one thread per output applies.  They meet in a
//             scratch buffer allocated at _create and walk a call in chunks of whole blocks that fit it.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"

// every operation of the contract is rounded on its own; the one product that may be fused (x x into a2, exact in double) is written
// as an fma explicitly
#pragma clang fp contract(off)

namespace {

constexpr int kFbMaxR = 4096, kFbMaxF = 16384, kFbMinTb = 16, kFbMaxTb = 4096;
constexpr int kFbSeg = 16;                       // segments per block = waves of the slab kernel
constexpr int kFbWave = 64;
constexpr int kFbThreads = kFbSeg * kFbWave;
constexpr int kFbCG = 256;                       // channels per group: 64 lanes x 16 bytes
constexpr int kFbMaxGroups = 16;                 // slab route: F <= 4096
constexpr int kFbStageBytes = kFbSeg * 2 * kFbCG * 8;
constexpr long long kFbMaxCall = 1ll << 40;
constexpr size_t kFbScratchBytes = (size_t)16 << 20;  // generic route: blocks per chunk = what fits this, at least one
constexpr long long kFbHostBytes = 8ll << 20;         // host path: input bytes per piece unless one block needs more

struct __attribute__((packed, aligned(4))) F4 { float v[4]; };  // 16 bytes at any 4-byte alignment

struct FbLim {
    double M;      // (double)Tb
    double c;      // (M nd + 1) / (M - 1)
    double sk_lo, sk_hi;
    double td2;    // td td
    int zero_dm;
};

struct FbArgs {
    int R, F, Tb, L, groups;
    long long units;  // (block, row) slabs of the call, row fastest
    FbLim lim;
};

__host__ __device__ inline double fb_tree16(const double *a)
{
    const double b0 = a[0] + a[1], b1 = a[2] + a[3], b2 = a[4] + a[5], b3 = a[6] + a[7];
    const double b4 = a[8] + a[9], b5 = a[10] + a[11], b6 = a[12] + a[13], b7 = a[14] + a[15];
    const double c0 = b0 + b1, c1 = b2 + b3, c2 = b4 + b5, c3 = b6 + b7;
    const double d0 = c0 + c1, d1 = c2 + c3;
    return d0 + d1;
}

__host__ __device__ inline double fb_sk(double s1, double s2, double M, double c)
{
    const double num = M * s2;
    const double den = s1 * s1;
    const double q = num / den;
    const double e = q - 1.0;
    return c * e;
}

// step 2 of the contract.  pos: var > 0, the condition under which stats carries {m32, is32} (else {+0, +0})
__device__ inline void fb_step2(double s1, double s2, const FbLim &lim, bool masked, float &m32, float &is32, bool &good)
{
    const double m = s1 / lim.M;
    const double e2 = s2 / lim.M;
    const double mm = m * m;
    const double var = e2 - mm;
    const double sk = fb_sk(s1, s2, lim.M, lim.c);
    const bool pos = var > 0.0;
    good = !masked && pos && sk >= lim.sk_lo && sk <= lim.sk_hi;
    m32 = pos ? (float)m : 0.0f;
    is32 = pos ? (float)(1.0 / sqrt(var)) : 0.0f;
}

// `in` and `out` may be the same buffer: no __restrict__ on either.  MG: the groups phase B keeps in registers, >= a.groups
template <int MG>
__global__ __launch_bounds__(kFbThreads) void k_fb_slab(const float *in, float *out, const uint8_t *__restrict__ mask, uint8_t *__restrict__ cflags,
                                                        uint8_t *__restrict__ tflags, float2 *__restrict__ stats, const FbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
    double *stage = (double *)fb_lds;                    // [segment][a1 | a2][256 channels of the group]
    float *lm = (float *)(fb_lds + kFbStageBytes);       // [F]
    float *lis = lm + a.F;                               // [F]
    uint8_t *lgood = (uint8_t *)(lis + a.F);             // [F]
    int *lng = (int *)(lgood + a.F);                     // good channels of the slab
    const int tid = threadIdx.x, lane = tid & (kFbWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kFbWave);
    const int R = a.R, F = a.F, Tb = a.Tb, L = a.L;
    const size_t rs = (size_t)R * F;                     // floats between time samples
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int r = (int)(u % R);
        const long long b = u / R;
        const size_t slab = ((size_t)b * Tb * R + r) * F;  // first float of the slab
        if (tid == 0) *lng = 0;
        // ---- phase A
        for (int g = 0; g < a.groups; g++) {
            const float *src = in + slab + (size_t)wave * L * rs + g * kFbCG + 4 * lane;
            double a1[4] = {0.0, 0.0, 0.0, 0.0}, a2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
            for (int i = 0; i < L; i++) {
                const F4 v = *(const F4 *)(src + (size_t)i * rs);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double d = (double)v.v[k];
                    a1[k] = a1[k] + d;
                    a2[k] = __builtin_fma(d, d, a2[k]);  // d d is exact in double
                }
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                stage[(wave * 2 + 0) * kFbCG + 4 * lane + k] = a1[k];
                stage[(wave * 2 + 1) * kFbCG + 4 * lane + k] = a2[k];
            }
            __syncthreads();
            if (tid < kFbCG) {
                const int f = g * kFbCG + tid;
                double t1[kFbSeg], t2[kFbSeg];
#pragma unroll
                for (int s = 0; s < kFbSeg; s++) {
                    t1[s] = stage[(s * 2 + 0) * kFbCG + tid];
                    t2[s] = stage[(s * 2 + 1) * kFbCG + tid];
                }
                float m32, is32;
                bool good;
                fb_step2(fb_tree16(t1), fb_tree16(t2), a.lim, mask[f] != 0, m32, is32, good);
                lm[f] = m32;
                lis[f] = is32;
                lgood[f] = good ? 1 : 0;
                const size_t cell = ((size_t)b * R + r) * F + f;
                if (cflags) cflags[cell] = good ? 0 : 1;
                if (stats) stats[cell] = make_float2(m32, is32);
                const int cnt = __popcll(__ballot(good));
                if (lane == 0) atomicAdd(lng, cnt);
            }
            __syncthreads();  // the stage is free again; after the last group: m32, is32, good and the count are complete
        }
        // ---- phase B
        const double ngd = (double)*lng;
        for (int i = 0; i < L; i++) {
            const int tl = i * kFbSeg + wave;
            const size_t row = slab + (size_t)tl * rs + 4 * lane;
            float y[MG][4];
            double p = 0.0;
#pragma unroll
            for (int g = 0; g < MG; g++) {
                if (g < a.groups) {  // (uniform)
                    const F4 v = *(const F4 *)(in + row + g * kFbCG);
                    const float4 m = *(const float4 *)(lm + g * kFbCG + 4 * lane);
                    const float4 is = *(const float4 *)(lis + g * kFbCG + 4 * lane);
                    const unsigned gd = *(const unsigned *)(lgood + g * kFbCG + 4 * lane);
                    const float mv[4] = {m.x, m.y, m.z, m.w}, iv[4] = {is.x, is.y, is.z, is.w};
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float d = v.v[k] - mv[k];
                        const float q = d * iv[k];
                        y[g][k] = ((gd >> (8 * k)) & 0xFFu) ? q : 0.0f;
                        if (a.lim.zero_dm) p = p + (double)y[g][k];  // (uniform)
                    }
                }
            }
            float z32 = 0.0f;
            bool tflag = false;
            if (a.lim.zero_dm) {
#pragma unroll
                for (int o = 1; o < kFbWave; o <<= 1) p = p + __shfl_xor(p, o, kFbWave);
                const double zz = p * p;
                const double lim = a.lim.td2 * ngd;
                tflag = zz > lim;
                z32 = (float)(p / ngd);
            }
            if (tflags && lane == 0) tflags[((size_t)b * Tb + tl) * R + r] = tflag ? 1 : 0;
#pragma unroll
            for (int g = 0; g < MG; g++) {
                if (g < a.groups) {  // (uniform)
                    F4 o;
                    if (a.lim.zero_dm) {
                        const unsigned gd = *(const unsigned *)(lgood + g * kFbCG + 4 * lane);
#pragma unroll
                        for (int k = 0; k < 4; k++) o.v[k] = (((gd >> (8 * k)) & 0xFFu) && !tflag) ? y[g][k] - z32 : 0.0f;
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; k++) o.v[k] = y[g][k];
                    }
                    *(F4 *)(out + row + g * kFbCG) = o;
                }
            }
        }
        __syncthreads();  // the next slab's phase A overwrites what phase B reads
    }
}

// ---- generic route.  Scratch of a chunk of nb blocks: st2[nb][R][F] float2 {m32, is32}, z[nb Tb][R] float, good[nb][R][F] uint8,
// tf[nb Tb][R] uint8.  The user's optional outputs start at the chunk's first block.
__global__ __launch_bounds__(256) void k_fb_stat(const float *in, const uint8_t *__restrict__ mask, float2 *__restrict__ st2, uint8_t *__restrict__ good,
                                                 uint8_t *__restrict__ cflags, float2 *__restrict__ stats, int R, int F, int Tb, long long nb, const FbLim lim)
{
    const long long total = nb * R * F;
    const size_t rs = (size_t)R * F;
    const int L = Tb / kFbSeg;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int f = (int)(i % F);
        const long long b = i / rs;
        const float *x = in + (size_t)b * Tb * rs + (size_t)(i % (long long)rs);
        double t1[kFbSeg], t2[kFbSeg];
#pragma unroll
        for (int s = 0; s < kFbSeg; s++) {
            double a1 = 0.0, a2 = 0.0;
            for (int k = 0; k < L; k++) {
                const double d = (double)x[(size_t)(s * L + k) * rs];
                a1 = a1 + d;
                a2 = __builtin_fma(d, d, a2);
            }
            t1[s] = a1;
            t2[s] = a2;
        }
        float m32, is32;
        bool g;
        fb_step2(fb_tree16(t1), fb_tree16(t2), lim, mask[f] != 0, m32, is32, g);
        st2[i] = make_float2(m32, is32);
        good[i] = g ? 1 : 0;
        if (cflags) cflags[i] = g ? 0 : 1;
        if (stats) stats[i] = make_float2(m32, is32);
    }
}

// one thread per (t, row) of the chunk
__global__ __launch_bounds__(256) void k_fb_zdm(const float *in, const float2 *__restrict__ st2, const uint8_t *__restrict__ good, float *__restrict__ z,
                                                uint8_t *__restrict__ tf, uint8_t *__restrict__ tflags, int R, int F, int Tb, long long nb, const FbLim lim)
{
    const long long total = nb * Tb * R;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        bool tflag = false;
        float z32 = 0.0f;
        if (lim.zero_dm) {
            const int r = (int)(i % R);
            const long long t = i / R, b = t / Tb;
            const float *x = in + (size_t)i * F;
            const size_t cell = ((size_t)b * R + r) * F;
            double p[kFbWave];
            int ng = 0;
            for (int j = 0; j < kFbWave; j++) {
                double acc = 0.0;
                for (int f0 = 4 * j; f0 < F; f0 += kFbCG)
                    for (int f = f0; f < f0 + 4 && f < F; f++)
                        if (good[cell + f]) {
                            const float2 s = st2[cell + f];
                            const float d = x[f] - s.x;
                            const float q = d * s.y;
                            acc = acc + (double)q;
                            ng++;
                        }
                p[j] = acc;
            }
            for (int w = kFbWave / 2; w >= 1; w >>= 1)
                for (int j = 0; j < w; j++) p[j] = p[2 * j] + p[2 * j + 1];
            const double zs = p[0], ngd = (double)ng;
            const double zz = zs * zs;
            const double bound = lim.td2 * ngd;
            tflag = zz > bound;
            z32 = (float)(zs / ngd);
        }
        z[i] = z32;
        tf[i] = tflag ? 1 : 0;
        if (tflags) tflags[i] = tflag ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_fb_apply(const float *in, float *out, const float2 *__restrict__ st2, const uint8_t *__restrict__ good,
                                                  const float *__restrict__ z, const uint8_t *__restrict__ tf, int R, int F, int Tb, long long nb,
                                                  int zero_dm)
{
    const size_t rs = (size_t)R * F;
    const long long total = nb * Tb * (long long)rs;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long tr = i / F, t = tr / R;
        const size_t cell = (size_t)(t / Tb) * rs + (size_t)(i % (long long)rs);
        float y = 0.0f;
        if (good[cell]) {
            const float2 s = st2[cell];
            const float d = in[i] - s.x;
            y = d * s.y;
            if (zero_dm) y = tf[tr] ? 0.0f : y - z[tr];
        }
        out[i] = y;
    }
}

// everything that can be told without a device
int fb_check(int R, int F, int Tb)
{
    MI355_REQUIRE(R >= 1 && R <= kFbMaxR, "num_rows must be 1 .. 4096");
    MI355_REQUIRE(F >= 1 && F <= kFbMaxF, "num_channels must be 1 .. 16384");
    MI355_REQUIRE(Tb >= kFbMinTb && Tb <= kFbMaxTb && Tb % kFbSeg == 0, "block_len must be a multiple of 16 in 16 .. 4096");
    return MI355_OK;
}

int fb_check_limits(double nd, double sk_lo, double sk_hi, double td, int zero_dm)
{
    MI355_REQUIRE(std::isfinite(nd) && nd > 0.0, "nd must be positive and finite");
    MI355_REQUIRE(sk_lo <= sk_hi, "sk_lo must not be above sk_hi (NaN is refused)");
    MI355_REQUIRE(td >= 0.0, "td must be >= 0 (NaN is refused)");
    MI355_REQUIRE(zero_dm == 0 || zero_dm == 1, "zero_dm must be 0 or 1");
    return MI355_OK;
}

double fb_factor(int Tb, double nd)
{
    const double M = (double)Tb;
    const double a = M * nd;
    const double b = a + 1.0;
    const double d = M - 1.0;
    return b / d;
}

}  // namespace

struct mi355_fbclean {
    mi355_ctx *ctx = nullptr;
    int R = 0, F = 0, Tb = 0;
    double nd = 1.0, sk_lo = -INFINITY, sk_hi = INFINITY, td = INFINITY;
    int zero_dm = 0;
    bool slab_ok = false, generic = false;
    long long chunk = 1;            // generic route: blocks per chunk
    std::vector<uint8_t> mask;
    mi355_tables dmask;
    DevWorkspace ws;                // generic route
    DevBuf d_x, d_aux;              // host path
    std::string route;
    std::mutex lock;
};

namespace {

bool fb_slab(const mi355_fbclean *h) { return h->slab_ok && !h->generic; }

void fb_name_route(mi355_fbclean *h)
{
    char buf[120];
    if (fb_slab(h)) snprintf(buf, sizeof buf, "slab R=%d F=%d Tb=%d fg=%d", h->R, h->F, h->Tb, kFbCG);
    else snprintf(buf, sizeof buf, "generic R=%d F=%d Tb=%d", h->R, h->F, h->Tb);
    h->route = buf;
}

FbLim fb_lim(const mi355_fbclean *h)
{
    FbLim l;
    l.M = (double)h->Tb;
    l.c = fb_factor(h->Tb, h->nd);
    l.sk_lo = h->sk_lo;
    l.sk_hi = h->sk_hi;
    l.td2 = h->td * h->td;
    l.zero_dm = h->zero_dm;
    return l;
}

size_t fb_scratch_per_block(const mi355_fbclean *h) { return (size_t)h->R * h->F * 9 + (size_t)h->Tb * h->R * 5 + 64; }

// caller holds the lock and has set the device; n > 0 is a multiple of Tb
int fb_launch(mi355_fbclean *h, long long n, const void *in, void *out, void *cflags, void *tflags, void *stats, hipStream_t st)
{
    const int R = h->R, F = h->F, Tb = h->Tb;
    const long long nblk = n / Tb;
    const uint8_t *d_mask = (const uint8_t *)h->dmask.current();
    const FbLim lim = fb_lim(h);
    if (fb_slab(h)) {
        FbArgs a = {};
        a.R = R; a.F = F; a.Tb = Tb; a.L = Tb / kFbSeg; a.groups = F / kFbCG;
        a.units = nblk * R;
        a.lim = lim;
        const int lds = kFbStageBytes + 9 * F + 16;
        const long long cap = (long long)mi355_cus(h->ctx) * 8;  // one resident workgroup of 16 waves per CU (by its registers), up to eight rounds
        const dim3 grid((unsigned)(a.units < cap ? a.units : cap));
        auto go = [&](auto kernel) -> int {
            MI355_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
            hipLaunchKernelGGL(kernel, grid, dim3(kFbThreads), (size_t)lds, st, (const float *)in, (float *)out, d_mask, (uint8_t *)cflags,
                               (uint8_t *)tflags, (float2 *)stats, a);
            MI355_HIP(hipGetLastError());
            return MI355_OK;
        };
        const int rc = a.groups <= 4 ? go(k_fb_slab<4>) : a.groups <= 8 ? go(k_fb_slab<8>) : go(k_fb_slab<kFbMaxGroups>);
        if (rc) return rc;
        return h->dmask.used(st);
    }
    int rc = h->ws.acquire(h->ws.bytes(), st);  // the size of _create: nothing is allocated here
    if (rc) return rc;
    const size_t cells = (size_t)h->chunk * R * F, samples = (size_t)h->chunk * Tb * R;
    char *w = (char *)h->ws.get();
    float2 *st2 = (float2 *)w;
    float *z = (float *)(w + cells * 8);
    uint8_t *good = (uint8_t *)(w + cells * 8 + samples * 4);
    uint8_t *tf = good + cells;
    const size_t rs = (size_t)R * F;
    for (long long b0 = 0; b0 < nblk; b0 += h->chunk) {
        const long long nb = nblk - b0 < h->chunk ? nblk - b0 : h->chunk;
        const float *x = (const float *)in + (size_t)b0 * Tb * rs;
        float *y = (float *)out + (size_t)b0 * Tb * rs;
        uint8_t *cf = cflags ? (uint8_t *)cflags + (size_t)b0 * rs : nullptr;
        float2 *sv = stats ? (float2 *)stats + (size_t)b0 * rs : nullptr;
        uint8_t *tv = tflags ? (uint8_t *)tflags + (size_t)b0 * Tb * R : nullptr;
        hipLaunchKernelGGL(k_fb_stat, dim3(mi355_grid_256(h->ctx, nb * (long long)rs, 32)), dim3(256), 0, st, x, d_mask, st2, good, cf, sv, R, F, Tb, nb, lim);
        hipLaunchKernelGGL(k_fb_zdm, dim3(mi355_grid_256(h->ctx, nb * Tb * R, 32)), dim3(256), 0, st, x, st2, good, z, tf, tv, R, F, Tb, nb, lim);
        hipLaunchKernelGGL(k_fb_apply, dim3(mi355_grid_256(h->ctx, nb * Tb * (long long)rs, 32)), dim3(256), 0, st, x, y, st2, good, z, tf, R, F, Tb, nb,
                           lim.zero_dm);
    }
    MI355_HIP(hipGetLastError());
    rc = h->ws.release(st);
    if (rc) return rc;
    return h->dmask.used(st);
}

int fb_args(const mi355_fbclean *h, long long n, const void *in, const void *out, const void *cflags, const void *tflags, const void *stats)
{
    MI355_REQUIRE(n >= 0, "n is negative");
    MI355_REQUIRE(n % h->Tb == 0, "n is not a multiple of block_len");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, "in must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, "out must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "stats must be 8-byte aligned");
    const long long per = 4ll * h->R * h->F;
    if (n > kFbMaxCall / per) {
        mi355_set_error("clFilterbankCleaner: %lld samples of %lld bytes in one call (the limit is 2^40 bytes per buffer)", n, per);
        return MI355_ERR_UNSUPPORTED;
    }
    const long long xb = n * per, nblk = n / h->Tb;
    MI355_REQUIRE(in == out || !mi355_overlap(in, xb, out, xb), "in and out overlap without being the same buffer");
    const void *p[4] = {out, cflags, tflags, stats};
    const long long pb[4] = {xb, nblk * h->R * h->F, n * h->R, 8 * nblk * h->R * h->F};
    for (int i = 1; i < 4; i++) {
        if (!p[i]) continue;
        MI355_REQUIRE(!mi355_overlap(in, xb, p[i], pb[i]), "in overlaps cflags, tflags or stats");
        for (int j = 0; j < i; j++) MI355_REQUIRE(!p[j] || !mi355_overlap(p[j], pb[j], p[i], pb[i]), "two outputs overlap");
    }
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_fbclean_plan(int num_rows, int num_channels, int block_len, long long *floats_per_sample, long long *cflag_bytes_per_block,
                                  long long *tflag_bytes_per_sample)
{
    if (floats_per_sample) *floats_per_sample = 0;
    if (cflag_bytes_per_block) *cflag_bytes_per_block = 0;
    if (tflag_bytes_per_sample) *tflag_bytes_per_sample = 0;
    const int rc = fb_check(num_rows, num_channels, block_len);
    if (rc) return rc;
    if (floats_per_sample) *floats_per_sample = (long long)num_rows * num_channels;
    if (cflag_bytes_per_block) *cflag_bytes_per_block = (long long)num_rows * num_channels;
    if (tflag_bytes_per_sample) *tflag_bytes_per_sample = num_rows;
    return MI355_OK;
}

extern "C" int mi355_fbclean_create(mi355_ctx *ctx, int num_rows, int num_channels, int block_len, double nd, double sk_lo, double sk_hi, double td,
                                    int zero_dm, const uint8_t *mask, mi355_fbclean **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    int rc = fb_check(num_rows, num_channels, block_len);
    if (rc) return rc;
    rc = fb_check_limits(nd, sk_lo, sk_hi, td, zero_dm);
    if (rc) return rc;
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_fbclean *h = new (std::nothrow) mi355_fbclean();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->R = num_rows; h->F = num_channels; h->Tb = block_len;
    h->nd = nd; h->sk_lo = sk_lo; h->sk_hi = sk_hi; h->td = td; h->zero_dm = zero_dm;
    h->slab_ok = h->F % kFbCG == 0 && h->F / kFbCG <= kFbMaxGroups;
    h->mask.assign((size_t)h->F, 0);
    if (mask)
        for (int f = 0; f < h->F; f++) h->mask[f] = mask[f] ? 1 : 0;
    const size_t per = fb_scratch_per_block(h);
    h->chunk = (long long)(kFbScratchBytes / per);
    if (h->chunk < 1) h->chunk = 1;
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_fbclean_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = h->dmask.publish(ctx, h->mask.data(), h->mask.size(), "mi355_fbclean: mask");
        if (rc == MI355_OK) rc = h->ws.acquire((size_t)h->chunk * per, ctx->stream[0]);
    }
    if (rc) { mi355_fbclean_destroy(h); return rc; }
    fb_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clFilterbankCleaner: %d rows, %d channels, blocks of %d: %s", h->R, h->F, h->Tb, h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_fbclean_destroy(mi355_fbclean *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    (void)h->ws.wait();
    h->ws.destroy();
    h->dmask.release();
    h->d_x.release();
    h->d_aux.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_fbclean_set_limits(mi355_fbclean *h, double nd, double sk_lo, double sk_hi, double td, int zero_dm)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = fb_check_limits(nd, sk_lo, sk_hi, td, zero_dm);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    h->nd = nd; h->sk_lo = sk_lo; h->sk_hi = sk_hi; h->td = td; h->zero_dm = zero_dm;
    return MI355_OK;
}

extern "C" int mi355_fbclean_get_limits(const mi355_fbclean *h, double *nd, double *sk_lo, double *sk_hi, double *td, int *zero_dm)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(const_cast<mi355_fbclean *>(h)->lock);
    if (nd) *nd = h->nd;
    if (sk_lo) *sk_lo = h->sk_lo;
    if (sk_hi) *sk_hi = h->sk_hi;
    if (td) *td = h->td;
    if (zero_dm) *zero_dm = h->zero_dm;
    return MI355_OK;
}

extern "C" int mi355_fbclean_set_mask(mi355_fbclean *h, const uint8_t *mask)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(mask != nullptr, "mask is NULL");
    std::vector<uint8_t> img((size_t)h->F);
    for (int f = 0; f < h->F; f++) img[f] = mask[f] ? 1 : 0;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const int rc = h->dmask.publish(h->ctx, img.data(), img.size(), "mi355_fbclean: mask");  // on failure the version in use stays
    if (rc) return rc;
    h->mask.swap(img);
    return MI355_OK;
}

extern "C" int mi355_fbclean_get_mask(const mi355_fbclean *h, uint8_t *out, long long cap_entries)
{
    MI355_REQUIRE(h && out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_fbclean *>(h)->lock);
    MI355_REQUIRE(cap_entries >= (long long)h->mask.size(), "out too small");
    memcpy(out, h->mask.data(), h->mask.size());
    return MI355_OK;
}

extern "C" long long mi355_fbclean_block_len(const mi355_fbclean *h) { return h ? h->Tb : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_fbclean_set_generic(mi355_fbclean *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    fb_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_fbclean_route(const mi355_fbclean *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_fbclean_work_dev(mi355_fbclean *h, long long n, const void *in, void *out, void *cflags, void *tflags, void *stats, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = fb_args(h, n, in, out, cflags, tflags, stats);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return fb_launch(h, n, in, out, cflags, tflags, stats, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_fbclean_work(mi355_fbclean *h, long long n, const void *in, void *out, void *cflags, void *tflags, void *stats)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = fb_args(h, n, in, out, cflags, tflags, stats);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole blocks, cleaned in place on the device; the flags and statistics of a piece lie behind one another in d_aux
    const long long R = h->R, F = h->F, Tb = h->Tb, nblk = n / Tb;
    const long long blk_bytes = 4 * Tb * R * F;
    const long long piece = mi355_piece_units(kFbHostBytes / blk_bytes, nblk);
    const size_t st_bytes = (size_t)(8 * piece * R * F), cf_bytes = (size_t)(piece * R * F), tf_bytes = (size_t)(piece * Tb * R);
    if ((rc = h->d_x.reserve((size_t)(piece * blk_bytes)))) return rc;
    if ((rc = h->d_aux.reserve(st_bytes + cf_bytes + tf_bytes))) return rc;
    char *d_st = (char *)h->d_aux.get(), *d_cf = d_st + st_bytes, *d_tf = d_cf + cf_bytes;
    return mi355_pageable_run(h->ctx, nblk, piece, [&](long long b0, long long nb, hipStream_t st) -> int {
        const size_t bytes = (size_t)(nb * blk_bytes);
        MI355_HIP(hipMemcpyAsync(h->d_x.get(), (const char *)in + (size_t)(b0 * blk_bytes), bytes, hipMemcpyHostToDevice, st));
        const int lrc = fb_launch(h, nb * Tb, h->d_x.get(), h->d_x.get(), cflags ? d_cf : nullptr, tflags ? d_tf : nullptr, stats ? d_st : nullptr, st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + (size_t)(b0 * blk_bytes), h->d_x.get(), bytes, hipMemcpyDeviceToHost, st));
        if (cflags) MI355_HIP(hipMemcpyAsync((char *)cflags + (size_t)(b0 * R * F), d_cf, (size_t)(nb * R * F), hipMemcpyDeviceToHost, st));
        if (tflags) MI355_HIP(hipMemcpyAsync((char *)tflags + (size_t)(b0 * Tb * R), d_tf, (size_t)(nb * Tb * R), hipMemcpyDeviceToHost, st));
        if (stats) MI355_HIP(hipMemcpyAsync((char *)stats + (size_t)(8 * b0 * R * F), d_st, (size_t)(8 * nb * R * F), hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
}

// host only: steps 1 and 2 of the contract on one column x[0], x[stride], ...
extern "C" int mi355_fbclean_sk_estimate(const float *x, int block_len, long long stride, double nd, double *sk)
{
    MI355_REQUIRE(x && sk, "NULL argument");
    MI355_REQUIRE(block_len >= kFbMinTb && block_len <= kFbMaxTb && block_len % kFbSeg == 0, "block_len must be a multiple of 16 in 16 .. 4096");
    MI355_REQUIRE(stride >= 1, "stride must be >= 1");
    MI355_REQUIRE(std::isfinite(nd) && nd > 0.0, "nd must be positive and finite");
    const int L = block_len / kFbSeg;
    double t1[kFbSeg], t2[kFbSeg];
    for (int s = 0; s < kFbSeg; s++) {
        double a1 = 0.0, a2 = 0.0;
        for (int k = 0; k < L; k++) {
            const double d = (double)x[(size_t)(s * L + k) * (size_t)stride];
            const double dd = d * d;
            a1 = a1 + d;
            a2 = a2 + dd;
        }
        t1[s] = a1;
        t2[s] = a2;
    }
    *sk = fb_sk(fb_tree16(t1), fb_tree16(t2), (double)block_len, fb_factor(block_len, nd));
    return MI355_OK;
}
