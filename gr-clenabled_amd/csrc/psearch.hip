// clPulseSearch: exact boxcar single-pulse search over the R D dedispersed time series that clDedisperser delivers, as gfx950 HIP
// kernels.  The contract is in include/mi355_clenabled.h; the reference module has no such block.
//
//     b_0[t] = x[t],   b_k[t] = b_(k-1)[t] + b_(k-1)[t + 2^(k-1)]        one binary32 addition each: a fixed balanced tree
//     snr_k[t] = (b_k[t] - mean 2^k) (inv_sigma c_k)                      one subtraction, one multiplication
//     peak of a (block of Tb outputs, series) = the largest 64-bit key {order-preserving map of snr's bits, ~((k << 24) | t)}
//
// The key and its kernels are peakkey.hpp's.  The peaks buffer itself carries the keys of a call: k_peak_init fills it with the empty
// key, the search kernel folds its keys in with 64-bit integer atomicMax, k_peak_emit decodes every key in place into its {snr, loc}
// record and compacts the records at or above the threshold into the candidate list (an integer counter).
//
// k_ps_tiled  the fused route.  A workgroup owns NS series x Tt = W - Hs outputs and stages the W samples of each in LDS (TRIAL_MAJOR:
//             NS = 1, contiguous runs; TIME_MAJOR: NS = 32, the 128-byte runs of 32 series per time sample, transposed into rows of
//             odd pitch W + 1: a wave's 32 + 32 stores fall on 32 banks each).  A thread owns positions tid + THREADS i of a row and keeps
//             its b_(k-1) there in registers; level k reads the partner at distance 2^(k-1) from LDS (a wave reads 64 consecutive
//             floats), all threads meet at a barrier, add, fold snr_k into the position's running (ordered snr, k) and store b_k back in
//             place behind a second barrier -- the reader and the writer of a slot are different threads.  The keys of a wave's 64
//             consecutive outputs are reduced with DPP row operations (ordered snr first, then loc) when they lie in one block, then per (series, block of the tile)
//             in LDS, then one global atomicMax per (series, block, tile).  Samples past the call's n + Hs are never read: they are
//             staged as zeros and reach only outputs t >= n, which are dropped.
// k_ps_gen    the generic route: one thread per output evaluates the tree of its widest boxcar leaf by leaf with a binary-counter
//             stack; the sums on the tree's left spine are the b_k[t] of every narrower width.  Any order, any K.
// k_ps_stats  mi355_psearch_measure: float64 mean and population variance per series, two passes, a fixed reduction order.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"
#include "peakkey.hpp"

#pragma clang fp contract(off)

namespace {

using peakkey::u64;

constexpr int kPsMaxR = 4096, kPsMaxD = 4096, kPsMaxK = 13, kPsMinTb = 16, kPsMaxTb = (1 << 24) - 1;
constexpr long long kPsMaxCall = 1ll << 40;
constexpr long long kPsHostBytes = 4ll << 20;   // host path: input bytes per staged piece unless one block needs more
constexpr int kPsLdsMax = 160 << 10;
constexpr int kPsTimeNS = 32;                    // series per workgroup of the TIME_MAJOR route: one 128-byte run per time sample

// snr_k of one sum folded into the running best of its output
__device__ __forceinline__ void ps_fold(float b, int k, float mean, float isg, unsigned &bo, unsigned &bk)
{
    const float m = mean * (float)(1 << k);
    const float g = isg * peakkey::c(k);
    const float d = b - m;
    peakkey::fold(d * g, k, bo, bk);
}

// record i of the [block][S series] peaks buffer
struct PsSplit {
    __device__ __forceinline__ uint2 operator()(long long i, int S) const { return make_uint2((unsigned)(i % S), (unsigned)(i / S)); }
};

struct PsArgs {
    int S, K, Tb, Tt, nbl;  // Tt = W - Hs outputs per tile; nbl: blocks a tile's outputs can touch
    unsigned tb_magic;      // floor(2^32 / Tb): x / Tb = mulhi(x, magic) or one more, for every 32-bit x
    long long n, ntot;      // outputs per series of the call, samples per series = n + Hs
    long long in_pitch;     // TRIAL_MAJOR
    long long ntt, groups;  // time tiles, series groups
    long long units;
};

// keys: the call's peaks buffer, [block][series] 64-bit keys (k_peak_init has filled it)
// stats: [mean S | inv_sigma S]
template <int ORDER, int THREADS, int NS, int EP, int CH>
__global__ __launch_bounds__(THREADS) void k_ps_tiled(const float *__restrict__ in, const float *__restrict__ stats, u64 *keys, const PsArgs a)
{
    constexpr int W = THREADS * EP, PITCH = NS == 1 ? W : W + 1, NE = NS * EP, PASSES = NE / CH;
    static_assert(NE % CH == 0 && (NS == 1 || EP == 1), "element plan");
    // [NS][nbl] keys, then the NS rows, then 2^(K-2) floats so that the widest partner read of the last row stays inside
    extern __shared__ __attribute__((aligned(16))) u64 lkeys[];
    float *lds = (float *)(lkeys + NS * a.nbl);
    const int tid = threadIdx.x, lane = tid & 63;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        // TRIAL_MAJOR: the tiles of a series are neighbours (they share their look-ahead in L2); TIME_MAJOR: the groups of a tile are
        const long long tile = ORDER == MI355_PSEARCH_TRIAL_MAJOR ? u % a.ntt : u / a.groups;
        const int s0 = ORDER == MI355_PSEARCH_TRIAL_MAJOR ? (int)(u / a.ntt) : (int)(u % a.groups) * NS;
        const long long t0 = tile * a.Tt;
        const long long tb0 = t0 / a.Tb;
        const unsigned rem0 = (unsigned)(t0 - tb0 * a.Tb);
        for (int i = tid; i < NS * a.nbl; i += THREADS) lkeys[i] = 0;
        const long long left = a.ntot - t0;  // samples from t0 to the end of the call's input, >= 1
        if (ORDER == MI355_PSEARCH_TRIAL_MAJOR) {
            const float *src = in + (size_t)s0 * (size_t)a.in_pitch + (size_t)t0;
#pragma unroll
            for (int i = 0; i < EP; i++) {
                const int p = tid + THREADS * i;
                lds[p] = p < left ? src[p] : 0.0f;
            }
        } else {
            const int j = tid & (NS - 1), tt = tid / NS;
            const bool has = s0 + j < a.S;
            const float *src = in + (size_t)t0 * (size_t)a.S + (size_t)(s0 + j);
#pragma unroll 8
            for (int i = 0; i < W / (THREADS / NS); i++) {
                const int p = tt + (THREADS / NS) * i;
                lds[j * PITCH + p] = (has && p < left) ? src[(size_t)p * (size_t)a.S] : 0.0f;
            }
        }
        __syncthreads();
        for (int pass = 0; pass < PASSES; pass++) {
            float r[CH], mean[CH], isg[CH];
            unsigned bo[CH], bk[CH];
            int row[CH];  // LDS index of the element
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const int e = pass * CH + c, j = e / EP, i = e % EP;
                const int s = s0 + j < a.S ? s0 + j : a.S - 1;
                row[c] = j * PITCH + tid + THREADS * i;
                mean[c] = stats[s];
                isg[c] = stats[a.S + s];
                r[c] = lds[row[c]];
                bo[c] = 0;
                bk[c] = 0;
                ps_fold(r[c], 0, mean[c], isg[c], bo[c], bk[c]);
            }
            for (int k = 1; k < a.K; k++) {
                const int h = 1 << (k - 1);
                float q[CH];
#pragma unroll
                for (int c = 0; c < CH; c++) q[c] = lds[row[c] + h];  // past the window: whatever lies behind the row; it reaches dropped outputs only
                __syncthreads();  // every partner has been read
#pragma unroll
                for (int c = 0; c < CH; c++) {
                    r[c] = r[c] + q[c];
                    ps_fold(r[c], k, mean[c], isg[c], bo[c], bk[c]);
                    lds[row[c]] = r[c];  // (the last level's store is not read again: one store in 2 K, no branch)
                }
                __syncthreads();  // level k is in place
            }
            // the keys of this pass: a wave holds 64 consecutive outputs of one series
#pragma unroll
            for (int c = 0; c < CH; c++) {
                const int e = pass * CH + c, j = e / EP, i = e % EP;
                const int p = tid + THREADS * i;
                const bool valid = p < a.Tt && t0 + p < a.n && s0 + j < a.S;
                const unsigned x = rem0 + (unsigned)p;
                unsigned bl = __umulhi(x, a.tb_magic), tin = x - bl * (unsigned)a.Tb;
                if (tin >= (unsigned)a.Tb) { bl++; tin -= (unsigned)a.Tb; }
                const unsigned o = valid ? bo[c] : 0u;  // 0: nothing to report
                const unsigned loc = (bk[c] << 24) | tin;
                const u64 live = __ballot(o != 0);
                if (live) {  // (uniform)
                    const int first = __ffsll((long long)live) - 1;
                    const unsigned bref = (unsigned)__builtin_amdgcn_readlane((int)bl, first);
                    if (__ballot(o != 0 && bl != bref) == 0) {
                        // one block: the largest ordered snr, then the smallest loc among the lanes that hold it (as k_ffa_pass, k_ss_tiled)
                        const unsigned mo = peakkey::wave_max(o);
                        const unsigned ml = peakkey::wave_min(o == mo ? loc : 0xFFFFFFFFu);
                        if (lane == first) atomicMax(&lkeys[j * a.nbl + (int)bref], peakkey::key(mo, ml));
                    } else if (o != 0) atomicMax(&lkeys[j * a.nbl + (int)bl], peakkey::key(o, loc));
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < NS * a.nbl; i += THREADS) {
            const u64 key = lkeys[i];
            if (key) {
                const int j = i / a.nbl, bl = i - j * a.nbl;
                atomicMax(&keys[(size_t)(tb0 + bl) * (size_t)a.S + (size_t)(s0 + j)], key);
            }
        }
        __syncthreads();  // lkeys and the rows are free for the next unit
    }
}

// generic route: one thread per output; TRIAL_MAJOR lanes along time, TIME_MAJOR lanes along the series
template <int ORDER>
__global__ __launch_bounds__(256) void k_ps_gen(const float *__restrict__ in, const float *__restrict__ stats, u64 *keys, int S, int K, int Tb,
                                                long long n, long long in_pitch)
{
    const long long total = (long long)S * n;
    const int width = 1 << (K - 1);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        long long t;
        int s;
        const float *x;
        size_t stride;
        if (ORDER == MI355_PSEARCH_TRIAL_MAJOR) {
            t = i % n; s = (int)(i / n);
            x = in + (size_t)s * (size_t)in_pitch + (size_t)t;
            stride = 1;
        } else {
            s = (int)(i % S); t = i / S;
            x = in + (size_t)t * (size_t)S + (size_t)s;
            stride = (size_t)S;
        }
        const float mean = stats[s], isg = stats[S + s];
        unsigned bo = 0, bk = 0;
        float st[kPsMaxK];
#pragma unroll
        for (int l = 0; l < kPsMaxK; l++) st[l] = 0.0f;
        // leaf j of the tree over x[t .. t + 2^(K-1)): merge while the counter carries.  The node finished at leaf 2^l - 1 is b_l[t]
        for (int j = 0; j < width; j++) {
            float v = x[(size_t)j * stride];
            bool open = true;
#pragma unroll
            for (int l = 0; l < kPsMaxK; l++) {
                if (open) {
                    if ((j >> l) & 1) v = st[l] + v;
                    else {
                        st[l] = v;
                        open = false;
                        if (j + 1 == (1 << l)) ps_fold(v, l, mean, isg, bo, bk);
                    }
                }
            }
        }
        if (bo != 0) {
            const long long b = t / Tb;
            atomicMax(&keys[(size_t)b * (size_t)S + (size_t)s], peakkey::key(bo, (bk << 24) | (unsigned)(t - b * Tb)));
        }
    }
}

// one workgroup per series: x[s sstride + t tstride], t < n; out [mean S | inv_sigma S]
__global__ __launch_bounds__(256) void k_ps_stats(const float *__restrict__ in, long long n, long long sstride, long long tstride, int S, float *out)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    auto total = [&](double v) {
        red[tid] = v;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) red[tid] = red[tid] + red[tid + w];
            __syncthreads();
        }
        const double sum = red[0];
        __syncthreads();
        return sum;
    };
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        const float *x = in + (size_t)s * (size_t)sstride;
        double acc = 0.0;
        for (long long t = tid; t < n; t += 256) acc += (double)x[(size_t)t * (size_t)tstride];
        const double mean = total(acc) / (double)n;
        acc = 0.0;
        for (long long t = tid; t < n; t += 256) {
            const double d = (double)x[(size_t)t * (size_t)tstride] - mean;
            acc += d * d;
        }
        const double var = total(acc) / (double)n;
        if (tid == 0) {
            out[s] = (float)mean;
            out[S + s] = var == 0.0 ? 0.0f : (float)(1.0 / sqrt(var));
        }
    }
}

// everything that can be told without a device
int psr_check(int R, int D, int K, int Tb, int order)
{
    MI355_REQUIRE(R >= 1 && R <= kPsMaxR, "num_rows must be 1 .. 4096");
    MI355_REQUIRE(D >= 1 && D <= kPsMaxD, "num_trials must be 1 .. 4096");
    MI355_REQUIRE(K >= 1 && K <= kPsMaxK, "num_widths must be 1 .. 13");
    MI355_REQUIRE(Tb >= kPsMinTb && Tb <= kPsMaxTb, "block_len must be 16 .. 2^24 - 1");
    MI355_REQUIRE(order == MI355_PSEARCH_TRIAL_MAJOR || order == MI355_PSEARCH_TIME_MAJOR, "order must be TRIAL_MAJOR (0) or TIME_MAJOR (1)");
    return MI355_OK;
}

}  // namespace

struct mi355_psearch {
    mi355_ctx *ctx = nullptr;
    int R = 0, D = 0, S = 0, K = 0, Tb = 0, Hs = 0, order = 0;
    int variant = 0;  // 0: outside the fused domain; 1 .. 3 TRIAL_MAJOR windows of 2048 / 4096 / 8192, 4 TIME_MAJOR 32 x 1024
    int W = 0, Tt = 0, nbl = 0, lds_bytes = 0;
    bool generic = false;
    float threshold = INFINITY;
    peakkey::SeriesStats stats;
    DevBuf d_in, d_out;        // host path
    std::string route;
    std::mutex lock;
};

namespace {

void psr_plan(mi355_psearch *h)
{
    const int K = h->K;
    int ns = 1;
    h->variant = 0;
    if (h->order == MI355_PSEARCH_TRIAL_MAJOR) {
        if (K <= 9) { h->variant = 1; h->W = 2048; }
        else if (K <= 11) { h->variant = 2; h->W = 4096; }
        else if (K == 12) { h->variant = 3; h->W = 8192; }
    } else if (K <= 10) { h->variant = 4; h->W = 1024; ns = kPsTimeNS; }
    if (!h->variant) return;
    h->Tt = h->W - h->Hs;
    h->nbl = (h->Tt + h->Tb - 2) / h->Tb + 1;  // blocks that Tt consecutive outputs can touch
    const int pitch = ns == 1 ? h->W : h->W + 1;
    h->lds_bytes = ns * h->nbl * 8 + (ns * pitch + (K >= 2 ? 1 << (K - 2) : 0)) * 4;
    if (h->lds_bytes > kPsLdsMax) h->variant = 0;
}

bool psr_fused(const mi355_psearch *h) { return h->variant != 0 && !h->generic; }

void psr_name_route(mi355_psearch *h)
{
    char buf[200];
    const char *ord = h->order == MI355_PSEARCH_TIME_MAJOR ? "time" : "trial";
    if (psr_fused(h))
        snprintf(buf, sizeof buf, "tiled %s R=%d D=%d K=%d Tb=%d ns=%d w=%d tt=%d", ord, h->R, h->D, h->K, h->Tb, h->variant == 4 ? kPsTimeNS : 1, h->W,
                 h->Tt);
    else snprintf(buf, sizeof buf, "generic %s R=%d D=%d K=%d Tb=%d", ord, h->R, h->D, h->K, h->Tb);
    h->route = buf;
}

template <int ORDER, int THREADS, int NS, int EP, int CH>
int psr_launch_tiled(const mi355_psearch *h, const PsArgs &a, int wg_per_cu, const float *in, const float *stats, u64 *keys, hipStream_t st)
{
    if (h->lds_bytes > (64 << 10))
        MI355_HIP(hipFuncSetAttribute((const void *)k_ps_tiled<ORDER, THREADS, NS, EP, CH>, hipFuncAttributeMaxDynamicSharedMemorySize, h->lds_bytes));
    const int cus = mi355_cus(h->ctx);
    const long long cap = (long long)cus * wg_per_cu * 4;  // four rounds of the resident workgroups
    const dim3 grid((unsigned)(a.units < cap ? a.units : cap));
    hipLaunchKernelGGL((k_ps_tiled<ORDER, THREADS, NS, EP, CH>), grid, dim3(THREADS), (size_t)h->lds_bytes, st, in, stats, keys, a);
    return MI355_OK;
}

// caller holds the lock and has set the device; n > 0 is a multiple of Tb
int psr_launch(mi355_psearch *h, long long n, const void *in, long long in_pitch, void *peaks, void *cands, long long max_cands, void *counts,
               hipStream_t st)
{
    const float *d_stats = h->stats.current();
    const long long nrec = n / h->Tb * h->S;
    const dim3 rec_grid(mi355_grid_256(h->ctx, nrec, 32));
    hipLaunchKernelGGL(peakkey::k_peak_init<>, rec_grid, dim3(256), 0, st, (u64 *)peaks, nrec, cands ? (unsigned *)counts : nullptr);
    if (psr_fused(h)) {
        PsArgs a = {};
        a.S = h->S; a.K = h->K; a.Tb = h->Tb; a.Tt = h->Tt; a.nbl = h->nbl;
        a.n = n; a.ntot = n + h->Hs; a.in_pitch = in_pitch;
        a.ntt = (n + h->Tt - 1) / h->Tt;
        a.groups = h->variant == 4 ? (h->S + kPsTimeNS - 1) / kPsTimeNS : h->S;
        a.units = a.ntt * a.groups;
        a.tb_magic = (unsigned)((1ull << 32) / (unsigned)h->Tb);
        int rc = MI355_OK;
        const float *x = (const float *)in;
        switch (h->variant) {
        case 1: rc = psr_launch_tiled<MI355_PSEARCH_TRIAL_MAJOR, 256, 1, 8, 8>(h, a, 8, x, d_stats, (u64 *)peaks, st); break;
        case 2: rc = psr_launch_tiled<MI355_PSEARCH_TRIAL_MAJOR, 512, 1, 8, 8>(h, a, 4, x, d_stats, (u64 *)peaks, st); break;
        case 3: rc = psr_launch_tiled<MI355_PSEARCH_TRIAL_MAJOR, 1024, 1, 8, 8>(h, a, 2, x, d_stats, (u64 *)peaks, st); break;
        default: rc = psr_launch_tiled<MI355_PSEARCH_TIME_MAJOR, 1024, kPsTimeNS, 1, 8>(h, a, 1, x, d_stats, (u64 *)peaks, st); break;
        }
        if (rc) return rc;
    } else {
        const dim3 grid(mi355_grid_256(h->ctx, n * h->S, 32));
        if (h->order == MI355_PSEARCH_TRIAL_MAJOR)
            hipLaunchKernelGGL(k_ps_gen<MI355_PSEARCH_TRIAL_MAJOR>, grid, dim3(256), 0, st, (const float *)in, d_stats, (u64 *)peaks, h->S, h->K, h->Tb, n,
                               in_pitch);
        else
            hipLaunchKernelGGL(k_ps_gen<MI355_PSEARCH_TIME_MAJOR>, grid, dim3(256), 0, st, (const float *)in, d_stats, (u64 *)peaks, h->S, h->K, h->Tb, n,
                               in_pitch);
    }
    hipLaunchKernelGGL(peakkey::k_peak_emit<PsSplit>, rec_grid, dim3(256), 0, st, (u64 *)peaks, nrec, h->S, h->threshold, (uint2 *)cands,
                       max_cands, (unsigned *)counts);
    MI355_HIP(hipGetLastError());
    return h->stats.used(st);  // this version of the statistics may be released behind these launches
}

// bytes from the first to one past the last float a call for n outputs reads
long long psr_in_bytes(const mi355_psearch *h, long long n, long long in_pitch)
{
    if (h->order == MI355_PSEARCH_TIME_MAJOR) return 4 * (n + h->Hs) * h->S;
    return 4 * ((long long)(h->S - 1) * in_pitch + n + h->Hs);
}

int psr_args(const mi355_psearch *h, long long n, const void *in, long long in_pitch, const void *peaks, const void *cands, long long max_cands,
             const void *counts)
{
    MI355_REQUIRE(n >= 0, "n is negative");
    MI355_REQUIRE(n % h->Tb == 0, "n is not a multiple of block_len");
    MI355_REQUIRE(max_cands >= 0, "max_cands is negative");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(in && peaks, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, "in must be 4-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(peaks) & 7u) == 0, "peaks must be 8-byte aligned");
    if (const int rc = peakkey::check_cands(cands, counts)) return rc;
    if (h->order == MI355_PSEARCH_TIME_MAJOR) MI355_REQUIRE(in_pitch == 0, "in_pitch must be 0 in TIME_MAJOR order");
    else MI355_REQUIRE(in_pitch >= n + h->Hs, "in_pitch is below n + history");
    const long long nblk = n / h->Tb;
    if (n > kPsMaxCall / (4ll * h->S) - h->Hs || in_pitch > kPsMaxCall / (4ll * h->S) || nblk > kPsMaxCall / (8ll * h->S) || nblk > 0xFFFFFFFFll ||
        max_cands > kPsMaxCall / 16) {
        mi355_set_error("clPulseSearch: %lld outputs of %d series, pitch %lld, %lld candidates in one call (the limit is 2^40 bytes per buffer)", n, h->S,
                        in_pitch, max_cands);
        return MI355_ERR_UNSUPPORTED;
    }
    const long long ib = psr_in_bytes(h, n, in_pitch), pb = 8 * nblk * h->S;
    MI355_REQUIRE(!mi355_overlap(in, ib, peaks, pb), "clPulseSearch does not work in place: in and peaks overlap");
    return peakkey::check_cands_apart(in, ib, peaks, pb, cands, max_cands, counts);
}

}  // namespace

extern "C" int mi355_psearch_plan(int num_rows, int num_trials, int num_widths, int block_len, int order, long long *in_floats_per_sample,
                                  long long *history, long long *peaks_per_block)
{
    if (in_floats_per_sample) *in_floats_per_sample = 0;
    if (history) *history = 0;
    if (peaks_per_block) *peaks_per_block = 0;
    const int rc = psr_check(num_rows, num_trials, num_widths, block_len, order);
    if (rc) return rc;
    if (in_floats_per_sample) *in_floats_per_sample = (long long)num_rows * num_trials;
    if (history) *history = (1ll << (num_widths - 1)) - 1;
    if (peaks_per_block) *peaks_per_block = (long long)num_rows * num_trials;
    return MI355_OK;
}

extern "C" int mi355_psearch_create(mi355_ctx *ctx, int num_rows, int num_trials, int num_widths, int block_len, int order, const float *mean,
                                    const float *inv_sigma, mi355_psearch **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    int rc = psr_check(num_rows, num_trials, num_widths, block_len, order);
    if (rc) return rc;
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_psearch *h = new (std::nothrow) mi355_psearch();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->R = num_rows; h->D = num_trials; h->S = num_rows * num_trials; h->K = num_widths; h->Tb = block_len; h->order = order;
    h->Hs = (1 << (num_widths - 1)) - 1;
    psr_plan(h);
    h->stats.init((size_t)h->S, mean, inv_sigma, "mi355_psearch: statistics");
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_psearch_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else rc = h->stats.publish(ctx);
    if (rc) { mi355_psearch_destroy(h); return rc; }
    psr_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clPulseSearch: %d rows, %d trials, %d widths, blocks of %d: %s", h->R, h->D, h->K, h->Tb, h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_psearch_destroy(mi355_psearch *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->stats.release();
    h->d_in.release();
    h->d_out.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_psearch_set_stats(mi355_psearch *h, const float *mean, const float *inv_sigma)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(mean && inv_sigma, "mean or inv_sigma is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return h->stats.set(h->ctx, mean, inv_sigma);
}

extern "C" int mi355_psearch_get_stats(const mi355_psearch *h, float *mean, float *inv_sigma, long long cap_entries)
{
    MI355_REQUIRE(h && mean && inv_sigma, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_psearch *>(h)->lock);
    MI355_REQUIRE(cap_entries >= (long long)h->S, "out too small");
    h->stats.get(mean, inv_sigma);
    return MI355_OK;
}

extern "C" int mi355_psearch_set_threshold(mi355_psearch *h, float threshold)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(threshold == threshold, "threshold is NaN");
    std::lock_guard<std::mutex> g(h->lock);
    h->threshold = threshold;
    return MI355_OK;
}

extern "C" long long mi355_psearch_history(const mi355_psearch *h) { return h ? h->Hs : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_psearch_set_generic(mi355_psearch *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    psr_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_psearch_route(const mi355_psearch *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_psearch_work_dev(mi355_psearch *h, long long n, const void *in, long long in_pitch, void *peaks, void *cands, long long max_cands,
                                      void *counts, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = psr_args(h, n, in, in_pitch, peaks, cands, max_cands, counts);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return psr_launch(h, n, in, in_pitch, peaks, cands, max_cands, counts, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_psearch_work(mi355_psearch *h, long long n, const void *in, long long in_pitch, void *peaks, void *cands, long long max_cands,
                                  void *counts)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = psr_args(h, n, in, in_pitch, peaks, cands, max_cands, counts);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole blocks, each sent with its Hs samples of look-ahead; the candidates of a piece come back in a list of their own
    // and are appended to the caller's with `block` counted from the call's first block
    const bool time_major = h->order == MI355_PSEARCH_TIME_MAJOR;
    const long long S = h->S, Tb = h->Tb, Hs = h->Hs, nblk = n / Tb;
    const long long piece = mi355_piece_units(kPsHostBytes / (4 * S * Tb), nblk);
    const size_t peak_bytes = (size_t)(8 * piece * S), cand_bytes = cands ? (size_t)(16 * max_cands) : 0;
    if ((rc = h->d_in.reserve((size_t)(4 * S * (piece * Tb + Hs))))) return rc;
    if ((rc = h->d_out.reserve(peak_bytes + 8 + cand_bytes))) return rc;
    char *d_peaks = (char *)h->d_out.get(), *d_counts = d_peaks + peak_bytes, *d_cands = d_counts + 8;
    peakkey::CandList list(cands, max_cands);
    rc = mi355_pageable_run(h->ctx, nblk, piece, [&](long long b0, long long nb, hipStream_t st) -> int {
        const long long m = nb * Tb, rows = m + Hs;
        if (time_major) MI355_HIP(hipMemcpyAsync(h->d_in.get(), (const float *)in + b0 * Tb * S, (size_t)(4 * rows * S), hipMemcpyHostToDevice, st));
        else
            MI355_HIP(hipMemcpy2DAsync(h->d_in.get(), (size_t)(4 * rows), (const float *)in + b0 * Tb, (size_t)(4 * in_pitch), (size_t)(4 * rows), (size_t)S,
                                       hipMemcpyHostToDevice, st));
        const int lrc = psr_launch(h, m, h->d_in.get(), time_major ? 0 : rows, d_peaks, cands ? d_cands : nullptr, max_cands, d_counts, st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)peaks + 8 * b0 * S, d_peaks, (size_t)(8 * nb * S), hipMemcpyDeviceToHost, st));
        return cands ? list.append(d_counts, d_cands, peakkey::CandList::BLOCK, b0, st) : MI355_OK;
    });
    if (rc) return rc;
    if (cands) list.finish(counts);
    return MI355_OK;
}

extern "C" int mi355_psearch_measure(mi355_psearch *h, long long n, const void *in, long long in_pitch, int in_is_device, float *mean, float *inv_sigma)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(n >= 1, "n must be at least 1");
    MI355_REQUIRE(in && mean && inv_sigma, "NULL argument");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0, "in must be 4-byte aligned");
    const bool time_major = h->order == MI355_PSEARCH_TIME_MAJOR;
    if (time_major) MI355_REQUIRE(in_pitch == 0, "in_pitch must be 0 in TIME_MAJOR order");
    else MI355_REQUIRE(in_pitch >= n, "in_pitch is below n");
    const long long S = h->S;
    if (n > kPsMaxCall / (4 * S) || in_pitch > kPsMaxCall / (4 * S)) {
        mi355_set_error("clPulseSearch: %lld samples of %lld series in one measurement (the limit is 2^40 bytes)", n, S);
        return MI355_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    hipStream_t st = h->ctx->stream[0];
    int rc = h->d_out.reserve((size_t)(8 * S));
    if (rc) return rc;
    const float *x = (const float *)in;
    long long pitch = in_pitch;
    if (!in_is_device) {
        if ((rc = h->d_in.reserve((size_t)(4 * S * n)))) return rc;
        if (time_major) MI355_HIP(hipMemcpyAsync(h->d_in.get(), in, (size_t)(4 * S * n), hipMemcpyHostToDevice, st));
        else MI355_HIP(hipMemcpy2DAsync(h->d_in.get(), (size_t)(4 * n), in, (size_t)(4 * in_pitch), (size_t)(4 * n), (size_t)S, hipMemcpyHostToDevice, st));
        x = (const float *)h->d_in.get();
        pitch = n;
    }
    const int cus = mi355_cus(h->ctx);
    const dim3 grid((unsigned)(S < (long long)cus * 8 ? S : (long long)cus * 8));
    hipLaunchKernelGGL(k_ps_stats, grid, dim3(256), 0, st, x, n, time_major ? 1ll : pitch, time_major ? S : 1ll, (int)S, (float *)h->d_out.get());
    std::vector<float> res(2 * (size_t)S);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), h->d_out.get(), (size_t)(8 * S), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);  // whatever was queued has finished before the scratch is given up
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) {
        mi355_set_error("mi355_psearch_measure: %s", hipGetErrorString(e));
        return MI355_ERR_HIP;
    }
    memcpy(mean, res.data(), (size_t)S * 4);
    memcpy(inv_sigma, res.data() + S, (size_t)S * 4);
    return MI355_OK;
}
