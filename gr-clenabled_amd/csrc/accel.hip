// clAccelResampler: exact acceleration trials for the period searches, as gfx950 HIP kernels.  Every dedispersed series is stretched
// quadratically once per trial; the copies are what clSpectralSearch, clPeriodSearch and clPulseSearch.measure() take as they lie.  The
// contract is in include/mi355_clenabled.h; the reference module has no such block.
//
//   d(i) = i (N - i);   delta_a(i) = floor((c[a] d(i) + 2^63) / 2^64);   src_a(i) = i + delta_a(i)
//   out[((s na) + (a - a0)) out_pitch + i] = in[s in_pitch + src_a(i)]
//
// The index is integer arithmetic throughout: c d is a signed 128-bit product, hi 2^64 + lo, and delta = hi + (lo >> 63).  Along a run
// of consecutive i the product is carried by its first and second differences, P(i+1) = P(i) + D(i), D(i) = c (N - 1 - 2 i),
// D(i+1) = D(i) - 2 c, all in 128 bits, and delta is taken from P at EVERY sample: d is concave, so equal shifts at the two ends of a
// run do not make the shift constant inside it.
//
// k_ac_tiled  the default route.  A workgroup owns (series, tile of 1024 outputs, group of consecutive trials).  src is non-decreasing
//             in i and, d being non-negative, in c, so the group's sources are the one contiguous window
//             [src_cmin(i0), src_cmax(i1)]; it is staged in LDS once (16-byte loads of whole aligned pieces, 4-byte ones at the ragged
//             ends: `in` may sit at any 4-byte alignment and nothing outside the window is read).  Then a wave writes one trial's tile
//             at a time: a lane owns runs of four outputs that start at a 16-byte boundary of `out` and leave as one 16-byte store.  A
//             trial's tile runs from boundary to boundary of its own output row (it starts up to three outputs before the nominal
//             tile), so only the outputs in front of a row's first boundary and behind its last leave as 4-byte stores.
// k_ac_gen    the generic route: one thread per output gathers from global memory.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"

namespace {

typedef unsigned long long u64;
typedef __int128 i128;

constexpr int kAcMaxS = 1 << 20, kAcMinN = 256, kAcMaxN = 1 << 22, kAcMaxA = 4096;
constexpr long long kAcMaxBytes = 1ll << 40;
constexpr long long kAcHostIn = 4ll << 20, kAcHostOut = 32ll << 20;  // host path: bytes per staged piece unless one series needs more
constexpr int kAcThreads = 256, kAcTile = 1024, kAcMaxGroup = 16;
// LDS words of a workgroup.  The window of a group at a tile holds at most
//     (T + 2) 3 / 2 + 2 + ceil((cmax - cmin) N^2 / 2^66)
// words: it serves outputs i0 - 3 .. i1, and src_cmax(i1) - src_cmin(i0 - 3) <= (T + 2) + x_cmax(i1) - x_cmin(i0 - 3) + 1 with
// x_c(i) = c d(i) / 2^64 (a shift is within 1/2 of it); |d(i1) - d(i0 - 3)| <= (T + 2) N and |c| N <= 2^63 give the first term,
// d <= N^2 / 4 the last.  It is placed 0 .. 3 words into the array.  kAcOneTrial is the bound without the last term: a group of one
// trial always fits.
constexpr int kAcLds = 4096;
constexpr int kAcOneTrial = (kAcTile + 2) * 3 / 2 + 2 + 3;
static_assert(kAcOneTrial < kAcLds, "a group of one trial must fit");
constexpr double kAcLight = 299792458.0;

// the shift of sample i: c d = hi 2^64 + lo, floor((c d + 2^63) / 2^64) = hi + (lo >> 63)
__host__ __device__ inline long long ac_delta(long long c, long long i, long long n)
{
    const i128 p = (i128)c * (i128)(i * (n - i)) + ((i128)1 << 63);
    return (long long)(p >> 64);
}

struct AcArgs {
    int n, na, a0, group, ngroups;
    long long tiles, in_pitch, out_pitch;
    long long units;  // series of the launch x tiles x groups
};

__global__ __launch_bounds__(kAcThreads) void k_ac_tiled(const unsigned *__restrict__ in, unsigned *__restrict__ out,
                                                         const long long *__restrict__ ctab, const AcArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned lds[kAcLds];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long n = a.n;
    for (long long u = blockIdx.x; u < a.units; u += gridDim.x) {
        const int g = (int)(u % a.ngroups);
        const long long r = u / a.ngroups, tile = r % a.tiles, s = r / a.tiles;
        const int t0 = g * a.group, G = a.na - t0 < a.group ? a.na - t0 : a.group;
        const long long i0 = tile * kAcTile;
        const int Tn = n - i0 < kAcTile ? (int)(n - i0) : kAcTile;
        const long long *cg = ctab + a.a0 + t0;
        long long cmin = cg[0], cmax = cg[0];
        for (int t = 1; t < G; t++) {
            const long long c = cg[t];
            cmin = c < cmin ? c : cmin;
            cmax = c > cmax ? c : cmax;
        }
        // the window: samples [lo, hi] of the series, placed (address of lo in words) & 3 words into the array, so that the 16-byte loads
        // and the 16-byte LDS stores are both aligned
        // (a trial's tile starts at the last 16-byte boundary of its output row at or before i0: up to three outputs earlier)
        const long long ilo = i0 >= 3 ? i0 - 3 : 0;
        const long long lo = ilo + ac_delta(cmin, ilo, n), hi = i0 + Tn - 1 + ac_delta(cmax, i0 + Tn - 1, n);
        const unsigned len = (unsigned)(hi - lo + 1);
        const unsigned *src = in + (size_t)s * (size_t)a.in_pitch + (size_t)lo;
        const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(src) >> 2) & 3u);
        const unsigned head = (4u - mis) & 3u;  // words before the first aligned one
        unsigned *dst = lds + mis;
        if (len <= head) {
            if ((unsigned)tid < len) dst[tid] = src[tid];
        } else {
            const unsigned nq = (len - head) >> 2, tail0 = head + 4 * nq;
            if ((unsigned)tid < head) dst[tid] = src[tid];
            if ((unsigned)tid < len - tail0) dst[tail0 + tid] = src[tail0 + tid];
            const uint4 *src4 = reinterpret_cast<const uint4 *>(src + head);
            uint4 *dst4 = reinterpret_cast<uint4 *>(dst + head);
            for (unsigned q = tid; q < nq; q += kAcThreads) dst4[q] = src4[q];
        }
        __syncthreads();
        for (int t = wave; t < G; t += kAcThreads / 64) {
            const long long c = cg[t];
            // this trial's tile: from the last 16-byte boundary of its row at or before i0 (the row's start for the first tile) to
            // the last one at or before i0 + Tn (the row's end for the last tile), so a tile of the middle is whole runs of four
            unsigned *row = out + ((size_t)s * (size_t)a.na + (size_t)(t0 + t)) * (size_t)a.out_pitch;
            const long long rw = (long long)(reinterpret_cast<uintptr_t>(row) >> 2);
            const long long b0 = i0 == 0 ? 0 : i0 - ((rw + i0) & 3), b1 = i0 + Tn == n ? n : i0 + Tn - ((rw + i0 + Tn) & 3);
            unsigned *o = row + (size_t)b0;
            const int Tt = (int)(b1 - b0);   // at most tile + 3
            const int w0 = (int)(b0 - lo);   // dst[w0 + k + delta] is the source of output b0 + k (always inside the window)
            const unsigned oh = (4u - (unsigned)((rw + b0) & 3)) & 3u;  // outputs before the first 16-byte boundary: the first tile only
            if ((unsigned)Tt <= oh) {
                if (lane < Tt) o[lane] = dst[w0 + lane + (int)ac_delta(c, b0 + lane, n)];
            } else {
                const unsigned nq = ((unsigned)Tt - oh) >> 2, tail0 = oh + 4 * nq;
                if ((unsigned)lane < oh) o[lane] = dst[w0 + lane + (int)ac_delta(c, b0 + lane, n)];
                if ((unsigned)lane < (unsigned)Tt - tail0) {  // the last tile only
                    const int k = (int)tail0 + lane;
                    o[k] = dst[w0 + k + (int)ac_delta(c, b0 + k, n)];
                }
                const i128 c2 = (i128)c * 2;
                for (unsigned q = lane; q < nq; q += 64) {
                    const int k = (int)(oh + 4 * q);
                    const long long i = b0 + k;
                    i128 P = (i128)c * (i128)(i * (n - i)) + ((i128)1 << 63);
                    i128 D = (i128)c * (i128)(n - 1 - 2 * i);
                    unsigned v[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        v[e] = dst[w0 + k + e + (int)(long long)(P >> 64)];
                        P += D;
                        D -= c2;
                    }
                    *reinterpret_cast<uint4 *>(o + k) = make_uint4(v[0], v[1], v[2], v[3]);
                }
            }
        }
        __syncthreads();  // the window is free for the next unit
    }
}

// generic route: one thread per output; a unit is 256 consecutive outputs of one row
__global__ __launch_bounds__(256) void k_ac_gen(const unsigned *__restrict__ in, unsigned *__restrict__ out, const long long *__restrict__ ctab,
                                                int n, int na, int a0, long long in_pitch, long long out_pitch, long long chunks, long long units)
{
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {
        const long long row = u / chunks, i = (u % chunks) * 256 + threadIdx.x;
        const long long s = row / na;
        const long long c = ctab[a0 + (int)(row % na)];
        if (i < n) out[(size_t)row * (size_t)out_pitch + (size_t)i] = in[(size_t)s * (size_t)in_pitch + (size_t)(i + ac_delta(c, i, n))];
    }
}

struct AcShape {
    int S, N, A;
};

// everything that can be told without a device
int ac_check(const AcShape &f)
{
    MI355_REQUIRE(f.S >= 1 && f.S <= kAcMaxS, "num_series must be 1 .. 2^20");
    MI355_REQUIRE(f.N >= kAcMinN && f.N <= kAcMaxN, "n must be 256 .. 2^22");
    MI355_REQUIRE(f.A >= 1 && f.A <= kAcMaxA, "num_trials must be 1 .. 4096");
    if ((long long)f.S * f.N > kAcMaxBytes / 4) {
        mi355_set_error("clAccelResampler: %d series of %d words (the limit is 2^40 bytes per buffer)", f.S, f.N);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

// |c| n <= 2^63
bool ac_coeff_ok(long long c, long long n)
{
    const unsigned __int128 m = c < 0 ? (unsigned __int128)(-(i128)c) : (unsigned __int128)c;
    return m * (unsigned __int128)n <= ((unsigned __int128)1 << 63);
}

int ac_check_table(const AcShape &f, const long long *c)
{
    for (int a = 0; a < f.A; a++)
        if (!ac_coeff_ok(c[a], f.N)) {
            mi355_set_error("invalid argument: trial %d: |c| n exceeds 2^63 (c = %lld, n = %d)", a, c[a], f.N);
            return MI355_ERR_INVALID_ARG;
        }
    return MI355_OK;
}

// words the spread of a group adds to its window: ceil((cmax - cmin) N^2 / 2^66)
long long ac_spread_words(long long cmin, long long cmax, long long n)
{
    const unsigned __int128 sp = (unsigned __int128)((i128)cmax - (i128)cmin);  // < 2^64 / n + 1
    const unsigned __int128 v = sp * (unsigned __int128)(n * n);                // < 2^87
    return (long long)((v + (((unsigned __int128)1 << 66) - 1)) >> 66);
}

// the largest group size, 1 .. 16, at which every run of that many consecutive trials fits the LDS budget (a call may start its
// groups at any trial)
int ac_group(const AcShape &f, const std::vector<long long> &c)
{
    int best = 1;
    for (int g = 2; g <= kAcMaxGroup && g <= f.A; g++) {
        bool fits = true;
        for (int a = 0; a + g <= f.A && fits; a++) {
            long long lo = c[(size_t)a], hi = lo;
            for (int t = 1; t < g; t++) {
                lo = c[(size_t)(a + t)] < lo ? c[(size_t)(a + t)] : lo;
                hi = c[(size_t)(a + t)] > hi ? c[(size_t)(a + t)] : hi;
            }
            fits = kAcOneTrial + ac_spread_words(lo, hi, f.N) <= kAcLds;
        }
        if (!fits) break;
        best = g;
    }
    return best;
}

}  // namespace

struct mi355_accel {
    mi355_ctx *ctx = nullptr;
    AcShape f = {};
    int group = 1;
    bool generic = false;
    std::vector<long long> trials;  // c[A]
    mi355_tables ttab;              // the same on the device (versioned)
    DevBuf d_in, d_out;             // host path
    std::string route;
    std::mutex lock;
};

namespace {

void ac_name_route(mi355_accel *h)
{
    char buf[160];
    if (h->generic) snprintf(buf, sizeof buf, "generic S=%d N=%d A=%d", h->f.S, h->f.N, h->f.A);
    else snprintf(buf, sizeof buf, "tiled S=%d N=%d A=%d tile=%d group=%d", h->f.S, h->f.N, h->f.A, kAcTile, h->group);
    h->route = buf;
}

// caller holds the lock and has set the device; nS series, trials a0 .. a0 + na - 1
int ac_launch(mi355_accel *h, long long nS, const void *in, long long in_pitch, void *out, long long out_pitch, int a0, int na, hipStream_t st)
{
    const long long *ctab = (const long long *)h->ttab.current();
    if (!h->generic) {
        AcArgs a = {};
        a.n = h->f.N; a.na = na; a.a0 = a0; a.group = h->group; a.ngroups = (na + h->group - 1) / h->group;
        a.tiles = (h->f.N + kAcTile - 1) / kAcTile; a.in_pitch = in_pitch; a.out_pitch = out_pitch;
        a.units = nS * a.tiles * a.ngroups;
        const long long cap = (long long)mi355_cus(h->ctx) * 8 * 4;  // four rounds of the resident workgroups
        hipLaunchKernelGGL(k_ac_tiled, dim3((unsigned)(a.units < cap ? a.units : cap)), dim3(kAcThreads), 0, st, (const unsigned *)in, (unsigned *)out,
                           ctab, a);
    } else {
        const long long chunks = (h->f.N + 255) / 256, units = nS * na * chunks;
        const long long cap = (long long)mi355_cus(h->ctx) * 32;
        hipLaunchKernelGGL(k_ac_gen, dim3((unsigned)(units < cap ? units : cap)), dim3(256), 0, st, (const unsigned *)in, (unsigned *)out, ctab,
                           h->f.N, na, a0, in_pitch, out_pitch, chunks, units);
    }
    MI355_HIP(hipGetLastError());
    return h->ttab.used(st);  // this version of the table may be released behind these launches
}

int ac_args(const mi355_accel *h, const void *in, long long in_pitch, const void *out, long long out_pitch, int a0, int na)
{
    const long long S = h->f.S, N = h->f.N;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE(a0 >= 0 && na >= 1 && a0 <= h->f.A - na, "the trial range must lie in 0 .. num_trials");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0, "in and out must be 4-byte aligned");
    MI355_REQUIRE(in_pitch >= N, "in_pitch is below the samples of a series");
    MI355_REQUIRE(out_pitch >= N, "out_pitch is below the samples of a series");
    if (in_pitch > kAcMaxBytes / (4 * S) || out_pitch > kAcMaxBytes / (4 * S * na)) {
        mi355_set_error("clAccelResampler: %lld series of pitch %lld, %lld rows of pitch %lld (the limit is 2^40 bytes per buffer)", S, in_pitch,
                        S * na, out_pitch);
        return MI355_ERR_UNSUPPORTED;
    }
    const long long ib = 4 * ((S - 1) * in_pitch + N), ob = 4 * ((S * na - 1) * out_pitch + N);
    MI355_REQUIRE(!mi355_overlap(in, ib, out, ob), "clAccelResampler does not work in place: in and out overlap");
    return MI355_OK;
}

// c of an acceleration in long double: round(-2^64 accel tsamp / (2 c_light)); false when it is not finite or leaves the bound
bool ac_coeff(long long n, long double tsamp, long double accel, long long *c)
{
    const long double v = -(accel * tsamp) / (2.0L * (long double)kAcLight) * 18446744073709551616.0L;
    if (!(fabsl(v) <= 9223372036854775807.0L)) return false;  // (also NaN); the bound is 2^63 / n <= 2^55
    const long long r = llroundl(v);
    if (!ac_coeff_ok(r, n)) return false;
    *c = r;
    return true;
}

bool ac_n_ok(int n) { return n >= kAcMinN && n <= kAcMaxN; }

}  // namespace

extern "C" int mi355_accel_plan(int num_series, int n, int num_trials, long long *rows, long long *tile, long long *table_bytes)
{
    if (rows) *rows = 0;
    if (tile) *tile = 0;
    if (table_bytes) *table_bytes = 0;
    const AcShape f = {num_series, n, num_trials};
    const int rc = ac_check(f);
    if (rc) return rc;
    if (rows) *rows = (long long)f.S * f.A;
    if (tile) *tile = kAcTile;
    if (table_bytes) *table_bytes = 8ll * f.A;
    return MI355_OK;
}

extern "C" int mi355_accel_create(mi355_ctx *ctx, int num_series, int n, int num_trials, const long long *c, mi355_accel **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    const AcShape f = {num_series, n, num_trials};
    int rc = ac_check(f);
    if (rc) return rc;
    if (c && (rc = ac_check_table(f, c))) return rc;
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_accel *h = new (std::nothrow) mi355_accel();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->f = f;
    h->trials.assign((size_t)f.A, 0ll);
    if (c) memcpy(h->trials.data(), c, (size_t)f.A * 8);
    h->group = ac_group(f, h->trials);
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_accel_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else rc = h->ttab.publish(ctx, h->trials.data(), (size_t)f.A * 8, "mi355_accel: trials");
    if (rc) { mi355_accel_destroy(h); return rc; }
    ac_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clAccelResampler: %d series of %d samples, %d trials: %s", f.S, f.N, f.A, h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_accel_destroy(mi355_accel *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->ttab.release();
    h->d_in.release();
    h->d_out.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_accel_set_trials(mi355_accel *h, const long long *c)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(c != nullptr, "c is NULL");
    int rc = ac_check_table(h->f, c);
    if (rc) return rc;
    std::vector<long long> img(c, c + h->f.A);
    const int group = ac_group(h->f, img);
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    rc = h->ttab.publish(h->ctx, img.data(), img.size() * 8, "mi355_accel: trials");  // on failure the version in use stays
    if (rc) return rc;
    h->trials.swap(img);
    h->group = group;
    ac_name_route(h);
    return MI355_OK;
}

extern "C" int mi355_accel_get_trials(const mi355_accel *h, long long *c, long long cap_entries)
{
    MI355_REQUIRE(h && c, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_accel *>(h)->lock);
    MI355_REQUIRE(cap_entries >= (long long)h->f.A, "out too small");
    memcpy(c, h->trials.data(), (size_t)h->f.A * 8);
    return MI355_OK;
}

extern "C" int mi355_accel_set_generic(mi355_accel *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    ac_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_accel_route(const mi355_accel *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_accel_work_dev(mi355_accel *h, const void *in, long long in_pitch, void *out, long long out_pitch, int a0, int na, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = ac_args(h, in, in_pitch, out, out_pitch, a0, na);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return ac_launch(h, h->f.S, in, in_pitch, out, out_pitch, a0, na, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_accel_work(mi355_accel *h, const void *in, long long in_pitch, void *out, long long out_pitch, int a0, int na)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = ac_args(h, in, in_pitch, out, out_pitch, a0, na);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole series, and per piece of series runs of whole trials: a unit of the piece loop is (piece of ps series, run of pa
    // trials), the runs of a piece behind one another, so the piece's input is copied in with its first run and stays for the others
    const long long S = h->f.S, N = h->f.N;
    const long long ps = mi355_piece_units(kAcHostIn / (4 * N), S);
    const long long pa = mi355_piece_units(kAcHostOut / (4 * N * ps), (long long)na);
    const long long runs = (na + pa - 1) / pa, pieces = (S + ps - 1) / ps;
    if ((rc = h->d_in.reserve((size_t)(4 * N * ps)))) return rc;
    if ((rc = h->d_out.reserve((size_t)(4 * N * ps * pa)))) return rc;
    return mi355_pageable_run(h->ctx, pieces * runs, 1ll, [&](long long unit, long long, hipStream_t st) -> int {
        const long long s0 = unit / runs * ps, ns = S - s0 < ps ? S - s0 : ps;
        const long long t0 = unit % runs * pa, nt = na - t0 < pa ? na - t0 : pa;
        if (t0 == 0)
            MI355_HIP(hipMemcpy2DAsync(h->d_in.get(), (size_t)(4 * N), (const uint32_t *)in + s0 * in_pitch, (size_t)(4 * in_pitch), (size_t)(4 * N),
                                       (size_t)ns, hipMemcpyHostToDevice, st));
        const int lrc = ac_launch(h, ns, h->d_in.get(), N, h->d_out.get(), N, a0 + (int)t0, (int)nt, st);
        if (lrc) return lrc;
        // the device rows [s][t] of the unit lie behind one another; the caller's rows of a series are na apart
        for (long long s = 0; s < (nt == na ? 1 : ns); s++) {
            uint32_t *dst = (uint32_t *)out + ((s0 + s) * na + t0) * out_pitch;
            MI355_HIP(hipMemcpy2DAsync(dst, (size_t)(4 * out_pitch), (const uint32_t *)h->d_out.get() + s * nt * N, (size_t)(4 * N), (size_t)(4 * N),
                                       (size_t)(nt == na ? ns * na : nt), hipMemcpyDeviceToHost, st));
        }
        return MI355_OK;
    });
}

// host only: the coefficient of an acceleration
extern "C" int mi355_accel_coeff(int n, double tsamp_s, double accel_m_s2, long long *c)
{
    MI355_REQUIRE(c != nullptr, "NULL argument");
    *c = 0;
    MI355_REQUIRE(ac_n_ok(n), "n must be 256 .. 2^22");
    MI355_REQUIRE(tsamp_s > 0.0 && std::isfinite(tsamp_s), "tsamp_s must be positive and finite");
    MI355_REQUIRE(std::isfinite(accel_m_s2), "accel_m_s2 must be finite");
    MI355_REQUIRE(ac_coeff(n, (long double)tsamp_s, (long double)accel_m_s2, c), "the coefficient leaves the bound |c| n <= 2^63");
    return MI355_OK;
}

// host only: src(i) for i0 <= i < i0 + count
extern "C" int mi355_accel_index(int n, long long c, long long i0, long long count, long long *src)
{
    MI355_REQUIRE(ac_n_ok(n), "n must be 256 .. 2^22");
    MI355_REQUIRE(ac_coeff_ok(c, n), "the coefficient leaves the bound |c| n <= 2^63");
    MI355_REQUIRE(i0 >= 0 && count >= 0 && i0 <= (long long)n - count, "the window must lie in 0 .. n");
    MI355_REQUIRE(src != nullptr || count == 0, "NULL argument");
    for (long long k = 0; k < count; k++) src[k] = i0 + k + ac_delta(c, i0 + k, n);
    return MI355_OK;
}

// host only: the ladder a_j = j da, da = tol 8 c_light / (tsamp n^2), for the integers j with a_lo <= a_j <= a_hi, ascending
extern "C" int mi355_accel_trials(int n, double tsamp_s, double a_lo, double a_hi, double tol_samples, long long *c, long long cap, long long *count)
{
    MI355_REQUIRE(count != nullptr, "NULL argument");
    *count = 0;
    MI355_REQUIRE(ac_n_ok(n), "n must be 256 .. 2^22");
    MI355_REQUIRE(tsamp_s > 0.0 && std::isfinite(tsamp_s), "tsamp_s must be positive and finite");
    MI355_REQUIRE(std::isfinite(a_lo) && std::isfinite(a_hi) && a_lo <= a_hi, "a_lo <= a_hi, both finite");
    MI355_REQUIRE(tol_samples > 0.0 && std::isfinite(tol_samples), "tol_samples must be positive and finite");
    MI355_REQUIRE(cap >= 0 && (c != nullptr || cap == 0), "cap is negative, or c is NULL with cap > 0");
    const long double da = (long double)tol_samples * 8.0L * (long double)kAcLight / ((long double)tsamp_s * (long double)n * (long double)n);
    long double jl = ceill((long double)a_lo / da), jh = floorl((long double)a_hi / da);
    MI355_REQUIRE(std::isfinite((double)da) && da > 0.0L && fabsl(jl) < 0x1p62L && fabsl(jh) < 0x1p62L, "the ladder is too long to count");
    // the quotients are rounded: the comparisons that define the ladder are made on j da itself
    while (jl * da < (long double)a_lo) jl += 1.0L;
    while ((jl - 1.0L) * da >= (long double)a_lo) jl -= 1.0L;
    while (jh * da > (long double)a_hi) jh -= 1.0L;
    while ((jh + 1.0L) * da <= (long double)a_hi) jh += 1.0L;
    if (jh < jl) return MI355_OK;
    long long ends[2];
    MI355_REQUIRE(ac_coeff(n, (long double)tsamp_s, jl * da, &ends[0]) && ac_coeff(n, (long double)tsamp_s, jh * da, &ends[1]),
                  "a trial of the ladder leaves the bound |c| n <= 2^63");
    const long long first = (long long)jl, total = (long long)jh - first + 1;
    for (long long k = 0; k < total && k < cap; k++) {
        c[k] = 0;  // j = 0 is the identity exactly
        if (first + k != 0) (void)ac_coeff(n, (long double)tsamp_s, (long double)(first + k) * da, &c[k]);
    }
    *count = total;
    return MI355_OK;
}
