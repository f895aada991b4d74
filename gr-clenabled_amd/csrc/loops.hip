// clSignalSource (NCO) and clCostasLoop (BPSK / QPSK carrier recovery) as gfx950 HIP kernels.
// Reference behaviour: lib/clSignalSource_impl.cc:113-237,329-415 and lib/clCostasLoop_impl.cc:112-232,525-596, both in their
// fp64-device branch (the one an MI355X takes); the semantics are restated in include/mi355_clenabled.h.
//
// k_sigsource   write-bound: one accurate double sincos per thread at a base index, the other kRot-1 items of the thread by ONE
//               rotation each of that base by host-computed (cos, sin)(k inc) -- never chained, so the error stays at a few double
//               ulps and vanishes in the float rounding.  16-byte nontemporal stores, scalar head / tail.  LITERAL = true is the
//               reference's one-sincos-per-item form: the comparison variant, and the path of the int output (a truncation shows
//               a double ulp).
// k_costas_lanes  one lane per stream over the channelizer's item-major layout: a wave-load of item i is one contiguous run.  The
//               loads of the next kAhead items are in flight while the current ones are consumed, so the serial chain per lane is
//               arithmetic only.
// k_costas_one  one stream, one wave: a tile of 64 items is loaded coalesced one tile ahead, every lane runs the recurrence
//               redundantly on the item broadcast from lane j (v_readlane), lane j keeps output j, and the tile is stored as one
//               512-byte run.  Nothing but sincos -> rotate -> detector -> loop update is on the dependent chain.
// Every rounding of the Costas recurrence is written out (fma, dmul, dadd, ddiv below, compiled with contraction off) and all
// paths share costas_step(), so any split of a stream into calls is bit-identical to one call.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include "common.h"

// No product may be fused into a following sum anywhere in this file, on the device or on the host: the roundings are the
// reference's, and prologue, main loop and tail of a kernel must round alike.
#pragma clang fp contract(off)

namespace {

__host__ __device__ __forceinline__ double dmul(double a, double b) { return a * b; }
__host__ __device__ __forceinline__ double dadd(double a, double b) { return a + b; }
__host__ __device__ __forceinline__ double ddiv(double a, double b) { return a / b; }

constexpr double kTwoPi = 6.28318530717958647692;

typedef unsigned u4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ signal source
constexpr int kSrcThreads = 256;
constexpr int kRot = 16;                           // items per thread
constexpr int kSrcTile = kSrcThreads * kRot;       // items per workgroup

struct SrcRot { double c[kRot], s[kRot]; };        // (cos, sin)(k inc), k = offset of a thread's item from its base item

// OUT: 0 complex (cos, sin), 1 float cos, 2 float sin, 3 int cos, 4 int sin
template <int OUT>
__device__ __forceinline__ unsigned src_word(double c, double s)
{
    if constexpr (OUT == 1) return __float_as_uint((float)c);
    else if constexpr (OUT == 2) return __float_as_uint((float)s);
    else if constexpr (OUT == 3) return (unsigned)(int)c;   // toward zero
    else return (unsigned)(int)s;
}

// item i0 + i of the call: d = pos + inc * (double)(i0 + i), value (cos d * amp, sin d * amp)
__device__ __forceinline__ void src_literal(double pos, double inc, double amp, unsigned long long idx, double &c, double &s)
{
    const double d = dadd(pos, dmul(inc, (double)idx));
    double sn, cs;
    sincos(d, &sn, &cs);
    c = dmul(cs, amp);
    s = dmul(sn, amp);
}

template <int OUT>
__device__ __forceinline__ void src_store1(void *out, size_t i, double c, double s)
{
    if constexpr (OUT == 0) ((float2 *)out)[i] = make_float2((float)c, (float)s);
    else ((unsigned *)out)[i] = src_word<OUT>(c, s);
}

// `out` + head items is 16-byte aligned; items [0, head) are written by the first threads of workgroup 0, the rest in tiles of
// kSrcTile items from `head` on.  A thread owns vectors q = 0 .. Q-1 of VEC items at tile + (q * kSrcThreads + t) * VEC.
template <int OUT, bool LITERAL>
__global__ __launch_bounds__(kSrcThreads) void k_sigsource(void *__restrict__ out, size_t n, unsigned head, unsigned long long i0,
                                                           double pos, double inc, double amp, SrcRot rot)
{
    constexpr int VEC = OUT == 0 ? 2 : 4, Q = kRot / VEC;
    const unsigned t = threadIdx.x;
    if (blockIdx.x == 0 && t < head && t < n) {
        double c, s;
        src_literal(pos, inc, amp, i0 + t, c, s);
        src_store1<OUT>(out, t, c, s);
    }
    const size_t first = (size_t)head + (size_t)blockIdx.x * kSrcTile + (size_t)t * VEC;
    if (first >= n) return;
    double c0 = 0.0, s0 = 0.0;
    if constexpr (!LITERAL) src_literal(pos, inc, amp, i0 + first, c0, s0);
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const size_t i = first + (size_t)q * kSrcThreads * VEC;
        if (i >= n) break;
        double c[VEC], s[VEC];
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            if constexpr (LITERAL) {
                src_literal(pos, inc, amp, i0 + i + e, c[e], s[e]);
            } else if (q == 0 && e == 0) {
                c[e] = c0; s[e] = s0;
            } else {  // (c0 + j s0)(rc + j rs)
                const double rc = rot.c[q * VEC + e], rs = rot.s[q * VEC + e];
                c[e] = fma(c0, rc, -dmul(s0, rs));
                s[e] = fma(s0, rc, dmul(c0, rs));
            }
        }
        if (i + VEC <= n) {
            u4v v;
            if constexpr (OUT == 0) {
                v.x = __float_as_uint((float)c[0]); v.y = __float_as_uint((float)s[0]);
                v.z = __float_as_uint((float)c[1]); v.w = __float_as_uint((float)s[1]);
            } else {
                v.x = src_word<OUT>(c[0], s[0]); v.y = src_word<OUT>(c[1], s[1]);
                v.z = src_word<OUT>(c[2], s[2]); v.w = src_word<OUT>(c[3], s[3]);
            }
            __builtin_nontemporal_store(v, (u4v *)((char *)out + i * (OUT == 0 ? 8 : 4)));
        } else {
#pragma unroll
            for (int e = 0; e < VEC; e++)
                if (i + e < n) src_store1<OUT>(out, i + e, c[e], s[e]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ Costas loop
struct CostasState { double phase, freq, error; };

// one item of lib/clCostasLoop_impl.cc:165-226 (fp64 + fma branch); o = the de-rotated item before its rounding to float
template <int ORDER>
__device__ __forceinline__ void costas_step(CostasState &st, float re_f, float im_f, double alpha, double beta, double &o_r, double &o_i)
{
    const double re = (double)re_f, im = (double)im_f;
    double n_i, n_r;
    sincos(-st.phase, &n_i, &n_r);
    o_r = fma(re, n_r, -dmul(im, n_i));
    o_i = fma(re, n_i, dmul(im, n_r));
    double e;
    if constexpr (ORDER == 2) {
        e = dmul(o_r, o_i);
    } else {
        const double a = o_r > 0.0 ? o_i : -o_i;   // (o_r > 0 ? 1 : -1) * o_i: exact
        const double b = o_i > 0.0 ? o_r : -o_r;
        e = dadd(a, -b);
    }
    e = dmul(0.5, dadd(fabs(dadd(e, 1.0)), -fabs(dadd(e, -1.0))));
    double freq = fma(beta, e, st.freq);
    double phase = dadd(st.phase, fma(alpha, e, freq));
    if (phase > kTwoPi || phase < -kTwoPi) {
        const double r = ddiv(phase, kTwoPi);
        phase = dmul(dadd(r, -(double)(int)r), kTwoPi);
    }
    freq = freq > 1.0 ? 1.0 : (freq < -1.0 ? -1.0 : freq);
    st.phase = phase; st.freq = freq; st.error = e;
}

constexpr int kAhead = 8;  // items of a lane whose loads are in flight while the previous kAhead are consumed

// state: phase[S], freq[S], error[S].  in / out / freq_out item-major: [i * S + s].
template <int ORDER>
__global__ __launch_bounds__(64) void k_costas_lanes(const float2 *__restrict__ in, float2 *__restrict__ out, float *__restrict__ freq_out,
                                                     double *__restrict__ state, int S, size_t n, double alpha, double beta)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;  // partial last wave (no barriers below)
    CostasState st = {state[s], state[S + s], state[2 * (size_t)S + s]};
    const float2 *p = in + s;
    float2 cur[kAhead], nxt[kAhead];
#pragma unroll
    for (int k = 0; k < kAhead; k++)
        if ((size_t)k < n) cur[k] = p[(size_t)k * S];
    for (size_t base = 0; base < n; base += kAhead) {
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            const size_t i = base + kAhead + k;
            if (i < n) nxt[k] = p[i * S];
        }
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            const size_t i = base + k;
            if (i < n) {
                double o_r, o_i;
                costas_step<ORDER>(st, cur[k].x, cur[k].y, alpha, beta, o_r, o_i);
                out[i * S + s] = make_float2((float)o_r, (float)o_i);
                if (freq_out) freq_out[i * S + s] = (float)st.freq;
            }
        }
#pragma unroll
        for (int k = 0; k < kAhead; k++) cur[k] = nxt[k];
    }
    state[s] = st.phase; state[S + s] = st.freq; state[2 * (size_t)S + s] = st.error;
}

__device__ __forceinline__ float lane_bcast(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int ORDER>
__global__ __launch_bounds__(64) void k_costas_one(const float2 *__restrict__ in, float2 *__restrict__ out, float *__restrict__ freq_out,
                                                   double *__restrict__ state, size_t n, double alpha, double beta)
{
    const int lane = threadIdx.x;
    CostasState st = {state[0], state[1], state[2]};  // wave-uniform: every lane runs the same recurrence
    float2 cur = make_float2(0.f, 0.f), nxt = make_float2(0.f, 0.f);
    if ((size_t)lane < n) cur = in[lane];
    for (size_t base = 0; base < n; base += 64) {
        if (base + 64 + lane < n) nxt = in[base + 64 + lane];  // one tile ahead: landed long before the tile below is done
        const int cnt = n - base < 64 ? (int)(n - base) : 64;
        float2 keep = make_float2(0.f, 0.f);
        float keep_f = 0.f;
        for (int j = 0; j < cnt; j++) {
            double o_r, o_i;
            costas_step<ORDER>(st, lane_bcast(cur.x, j), lane_bcast(cur.y, j), alpha, beta, o_r, o_i);
            if (lane == j) { keep = make_float2((float)o_r, (float)o_i); keep_f = (float)st.freq; }
        }
        if (lane < cnt) {
            out[base + lane] = keep;
            if (freq_out) freq_out[base + lane] = keep_f;
        }
        cur = nxt;
    }
    if (lane == 0) { state[0] = st.phase; state[1] = st.freq; state[2] = st.error; }
}

// GNU Radio's control_loop gains (gr::blocks::control_loop::update_gains), float arithmetic
void costas_gains(float bw, float *alpha, float *beta)
{
    const float damp = sqrtf(2.0f) / 2.0f;
    const float denom = 1.0f + 2.0f * damp * bw + bw * bw;
    *alpha = (4.0f * damp * bw) / denom;
    *beta = (4.0f * bw * bw) / denom;
}

double wrap_2pi(double pos)  // lib/clSignalSource_impl.cc:386-399
{
    if (pos > kTwoPi || pos < -kTwoPi) {
        const double r = pos / kTwoPi;
        const double frac = r - (double)(int)r;
        pos = frac * kTwoPi;
    }
    return pos;
}

bool env_set(const char *name)
{
    const char *e = getenv(name);
    return e && atoi(e) > 0;
}

constexpr size_t kHostChunkItems = (size_t)1 << 21;  // staging chunk of the host-pointer paths (items over all streams)

}  // namespace

// ================================================================================================ clSignalSource
struct mi355_sigsource {
    mi355_ctx *ctx = nullptr;
    int dtype = 0, waveform = 0;
    double samp_rate = 0, freq = 0, amp = 0;
    double pos = 0, inc = 0;
    std::mutex lock;
    bool literal = false;    // one sincos per item: int output always; MI355_SIGSOURCE_LITERAL=1 at create (comparison variant)
    DevBuf d_buf;            // host path staging
};

namespace {

int sigsource_launch(mi355_sigsource *h, size_t n, unsigned long long i0, double pos, void *out, hipStream_t st)
{
    const size_t isz = h->dtype == MI355_DTYPE_COMPLEX ? 8 : 4;
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & (isz - 1)) == 0, "output buffer must be aligned to its item size");
    const unsigned head = (unsigned)(((16 - (reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / isz);
    const size_t body = n > head ? n - head : 0;
    const size_t tiles = (body + kSrcTile - 1) / kSrcTile;
    if (tiles > 0x7fffffffull) {
        mi355_set_error("clSignalSource: %zu items in one call", n);
        return MI355_ERR_UNSUPPORTED;
    }
    const unsigned grid = tiles ? (unsigned)tiles : 1u;
    const bool literal = h->literal;
    const int vec = h->dtype == MI355_DTYPE_COMPLEX ? 2 : 4;
    SrcRot rot;
    for (int q = 0; q < kRot / vec; q++)
        for (int e = 0; e < vec; e++) {
            const double a = h->inc * (double)(q * kSrcThreads * vec + e);
            rot.c[q * vec + e] = cos(a);
            rot.s[q * vec + e] = sin(a);
        }
    const int o = h->dtype == MI355_DTYPE_COMPLEX ? 0 : (h->dtype == MI355_DTYPE_FLOAT ? 0 : 2) + h->waveform;
#define SRC_CASE(OUT, LIT)                                                                                              \
    if (o == OUT && literal == LIT) {                                                                                   \
        hipLaunchKernelGGL((k_sigsource<OUT, LIT>), dim3(grid), dim3(kSrcThreads), 0, st, out, n, head, i0, pos, h->inc, h->amp, rot); \
    } else
    SRC_CASE(0, false) SRC_CASE(0, true) SRC_CASE(1, false) SRC_CASE(1, true) SRC_CASE(2, false) SRC_CASE(2, true)
    SRC_CASE(3, true) SRC_CASE(4, true) { return MI355_ERR_UNSUPPORTED; }
#undef SRC_CASE
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

void sigsource_advance(mi355_sigsource *h, size_t n)  // :386-399 (the item count passes through a float there)
{
    const double step = h->inc * (double)(float)n;
    h->pos = wrap_2pi(h->pos + step);
}

double sigsource_inc(double freq, double samp_rate)
{
    const double w = kTwoPi * freq;
    return w / samp_rate;
}

}  // namespace

extern "C" int mi355_sigsource_create(mi355_ctx *ctx, int dtype, double samp_rate, int waveform, double freq, float amplitude,
                                      mi355_sigsource **out)
{
    MI355_REQUIRE(ctx && out, "NULL argument");
    *out = nullptr;
    MI355_REQUIRE(dtype == MI355_DTYPE_COMPLEX || dtype == MI355_DTYPE_FLOAT || dtype == MI355_DTYPE_INT,
                  "clSignalSource dtype must be complex, float or int");
    MI355_REQUIRE(waveform == 1 || waveform == 2, "clSignalSource waveform must be 1 (cos) or 2 (sin)");
    MI355_REQUIRE(samp_rate != 0.0 && samp_rate == samp_rate, "clSignalSource samp_rate must not be 0");
    mi355_sigsource *h = new (std::nothrow) mi355_sigsource();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->dtype = dtype; h->waveform = waveform; h->samp_rate = samp_rate; h->freq = freq; h->amp = (double)amplitude;
    h->inc = sigsource_inc(freq, samp_rate);
    h->literal = dtype == MI355_DTYPE_INT || env_set("MI355_SIGSOURCE_LITERAL");
    mi355_log(ctx, MI355_LOG_INFO, "clSignalSource: %s, %s, %g Hz at %g S/s, amplitude %g, %s",
              dtype == MI355_DTYPE_COMPLEX ? "complex" : dtype == MI355_DTYPE_FLOAT ? "float" : "int", waveform == 1 ? "cos" : "sin",
              freq, samp_rate, (double)amplitude, h->literal ? "literal (one sincos per item)" : "rotation (one sincos per 16 items)");
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_sigsource_destroy(mi355_sigsource *h)
{
    if (!h) return MI355_OK;
    if (h->d_buf.get()) {
        (void)hipSetDevice(h->ctx->device);
        h->d_buf.release();
    }
    delete h;
    return MI355_OK;
}

extern "C" int mi355_sigsource_set_frequency(mi355_sigsource *h, double freq)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->freq = freq;
    h->inc = sigsource_inc(freq, h->samp_rate);  // the phase is kept
    return MI355_OK;
}

extern "C" int mi355_sigsource_get_state(const mi355_sigsource *h, double *angle_pos, double *angle_rate)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(const_cast<mi355_sigsource *>(h)->lock);
    if (angle_pos) *angle_pos = h->pos;
    if (angle_rate) *angle_rate = h->inc;
    return MI355_OK;
}

extern "C" int mi355_sigsource_set_phase(mi355_sigsource *h, double angle_pos)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(std::isfinite(angle_pos), "phase must be finite");
    std::lock_guard<std::mutex> g(h->lock);
    h->pos = angle_pos;
    return MI355_OK;
}

extern "C" int mi355_sigsource_work_dev(mi355_sigsource *h, size_t n, void *out_dev, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(out_dev != nullptr, "NULL buffer");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const int rc = sigsource_launch(h, n, 0, h->pos, out_dev, mi355_pick_stream(h->ctx, stream));
    if (rc) return rc;
    sigsource_advance(h, n);  // the phase is a kernel argument: calls are stream-ordered with no device state
    return MI355_OK;
}

extern "C" int mi355_sigsource_work(mi355_sigsource *h, size_t n, void *out_host)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (n == 0) return MI355_OK;
    MI355_REQUIRE(out_host != nullptr, "NULL buffer");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const size_t isz = h->dtype == MI355_DTYPE_COMPLEX ? 8 : 4;
    const size_t chunk = mi355_piece_units(kHostChunkItems, n);
    int rc = h->d_buf.reserve(chunk * isz);
    if (rc) return rc;
    rc = mi355_pageable_run(h->ctx, n, chunk, [&](size_t off, size_t m, hipStream_t st) -> int {
        const int lrc = sigsource_launch(h, m, off, h->pos, h->d_buf.get(), st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out_host + off * isz, h->d_buf.get(), m * isz, hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
    if (rc) return rc;
    sigsource_advance(h, n);
    return MI355_OK;
}

// ================================================================================================ clCostasLoop
struct mi355_costas {
    mi355_ctx *ctx = nullptr;
    int order = 0, S = 0;
    float bw = 0, alpha = 0, beta = 0;
    double *d_state = nullptr;       // phase[S], freq[S], error[S]
    hipEvent_t done = nullptr;       // the handle's last call
    hipStream_t last = nullptr;
    bool used = false;
    bool one_lane = false;           // MI355_COSTAS_ONE_LANE=1 at create: a single stream through k_costas_lanes (comparison variant)
    std::mutex lock;
    DevBuf d_in, d_out, d_freq;      // host path staging
};

namespace {

int costas_check(float loop_bw, int order)
{
    MI355_REQUIRE(order == 2 || order == 4, "clCostasLoop order must be 2 or 4");
    MI355_REQUIRE(loop_bw >= 0.0f && std::isfinite(loop_bw), "clCostasLoop loop_bw must not be negative");
    return MI355_OK;
}

// caller holds h->lock and has set the device
int costas_launch(mi355_costas *h, size_t nitems, const void *in, void *out, float *freq, hipStream_t st)
{
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0,
                  "device buffers must be 8-byte aligned");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(freq) & 3u) == 0, "frequency buffer must be 4-byte aligned");
    MI355_REQUIRE(in != out, "clCostasLoop does not work in place");
    if (h->used && h->last != st) MI355_HIP(hipStreamWaitEvent(st, h->done, 0));  // calls of one handle run in submission order
    const double alpha = (double)h->alpha, beta = (double)h->beta;
    const bool lanes = h->S > 1 || h->one_lane;
    if (lanes) {
        const dim3 grid((h->S + 63) / 64);
        if (h->order == 2)
            hipLaunchKernelGGL(k_costas_lanes<2>, grid, dim3(64), 0, st, (const float2 *)in, (float2 *)out, freq, h->d_state, h->S, nitems, alpha, beta);
        else
            hipLaunchKernelGGL(k_costas_lanes<4>, grid, dim3(64), 0, st, (const float2 *)in, (float2 *)out, freq, h->d_state, h->S, nitems, alpha, beta);
    } else {
        if (h->order == 2)
            hipLaunchKernelGGL(k_costas_one<2>, dim3(1), dim3(64), 0, st, (const float2 *)in, (float2 *)out, freq, h->d_state, nitems, alpha, beta);
        else
            hipLaunchKernelGGL(k_costas_one<4>, dim3(1), dim3(64), 0, st, (const float2 *)in, (float2 *)out, freq, h->d_state, nitems, alpha, beta);
    }
    MI355_HIP(hipGetLastError());
    MI355_HIP(hipEventRecord(h->done, st));
    h->last = st;
    h->used = true;
    return MI355_OK;
}

void costas_free(mi355_costas *h)
{
    (void)hipSetDevice(h->ctx->device);
    if (h->d_state) (void)hipFree(h->d_state);
    for (DevBuf *b : {&h->d_in, &h->d_out, &h->d_freq}) b->release();
    if (h->done) (void)hipEventDestroy(h->done);
    delete h;
}

}  // namespace

extern "C" int mi355_costas_plan(float loop_bw, int order, float *alpha, float *beta)
{
    if (alpha) *alpha = 0.0f;
    if (beta) *beta = 0.0f;
    const int rc = costas_check(loop_bw, order);
    if (rc) return rc;
    float a, b;
    costas_gains(loop_bw, &a, &b);
    if (alpha) *alpha = a;
    if (beta) *beta = b;
    return MI355_OK;
}

extern "C" int mi355_costas_create(mi355_ctx *ctx, float loop_bw, int order, int num_streams, mi355_costas **out)
{
    MI355_REQUIRE(ctx && out, "NULL argument");
    *out = nullptr;
    int rc = costas_check(loop_bw, order);
    if (rc) return rc;
    if (num_streams < 1 || num_streams > 4096) {
        mi355_set_error("clCostasLoop: num_streams %d outside 1 .. 4096", num_streams);
        return MI355_ERR_UNSUPPORTED;
    }
    mi355_costas *h = new (std::nothrow) mi355_costas();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->order = order; h->S = num_streams; h->bw = loop_bw;
    costas_gains(loop_bw, &h->alpha, &h->beta);
    h->one_lane = env_set("MI355_COSTAS_ONE_LANE");
    const size_t bytes = (size_t)3 * num_streams * sizeof(double);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&h->d_state, bytes);
    if (e == hipSuccess) e = mi355_fill(ctx, h->d_state, 0, bytes);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        mi355_set_error("mi355_costas_create: %s", hipGetErrorString(e));
        costas_free(h);
        return MI355_ERR_HIP;
    }
    mi355_log(ctx, MI355_LOG_INFO, "clCostasLoop: order %d, loop bandwidth %g (alpha %.9g, beta %.9g), %d stream%s, %s", order,
              (double)loop_bw, (double)h->alpha, (double)h->beta, num_streams, num_streams == 1 ? "" : "s",
              num_streams > 1 || h->one_lane ? "k_costas_lanes" : "k_costas_one");
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_costas_destroy(mi355_costas *h)
{
    if (!h) return MI355_OK;
    if (h->used) (void)hipEventSynchronize(h->done);
    costas_free(h);
    return MI355_OK;
}

extern "C" int mi355_costas_set_loop_bandwidth(mi355_costas *h, float loop_bw)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = costas_check(loop_bw, h->order);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    h->bw = loop_bw;
    costas_gains(loop_bw, &h->alpha, &h->beta);  // kernel arguments of the calls from here on
    return MI355_OK;
}

extern "C" int mi355_costas_get_state(mi355_costas *h, double *phase, double *freq, double *error)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    if (h->used) MI355_HIP(hipEventSynchronize(h->done));
    double *dst[3] = {phase, freq, error};
    std::lock_guard<std::mutex> gu(h->ctx->upload_lock);
    for (int k = 0; k < 3; k++)
        if (dst[k])
            MI355_HIP(hipMemcpyAsync(dst[k], h->d_state + (size_t)k * h->S, (size_t)h->S * sizeof(double), hipMemcpyDeviceToHost, h->ctx->upload));
    MI355_HIP(hipStreamSynchronize(h->ctx->upload));
    return MI355_OK;
}

extern "C" int mi355_costas_set_state(mi355_costas *h, const double *phase, const double *freq)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    if (h->used) MI355_HIP(hipEventSynchronize(h->done));  // the handle's last call has read and written the state
    const double *src[2] = {phase, freq};
    for (int k = 0; k < 2; k++)
        if (src[k]) MI355_HIP(mi355_upload(h->ctx, h->d_state + (size_t)k * h->S, src[k], (size_t)h->S * sizeof(double)));
    return MI355_OK;
}

extern "C" int mi355_costas_work_dev(mi355_costas *h, size_t nitems, const void *in_dev, void *out_dev, float *freq_dev, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (nitems == 0) return MI355_OK;
    MI355_REQUIRE(in_dev && out_dev, "NULL buffer");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return costas_launch(h, nitems, in_dev, out_dev, freq_dev, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_costas_work(mi355_costas *h, size_t nitems, const void *in, void *out, float *freq_out)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    if (nitems == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const size_t S = (size_t)h->S;
    const size_t chunk = mi355_piece_units(kHostChunkItems / S, nitems);  // items per stream and piece; any split gives the same bits
    int rc;
    if ((rc = h->d_in.reserve(chunk * S * 8)) || (rc = h->d_out.reserve(chunk * S * 8)) || (rc = h->d_freq.reserve(chunk * S * 4))) return rc;
    return mi355_pageable_run(h->ctx, nitems, chunk, [&](size_t off, size_t m, hipStream_t st) -> int {
        MI355_HIP(hipMemcpyAsync(h->d_in.get(), (const char *)in + off * S * 8, m * S * 8, hipMemcpyHostToDevice, st));
        const int lrc = costas_launch(h, m, h->d_in.get(), h->d_out.get(), freq_out ? (float *)h->d_freq.get() : nullptr, st);
        if (lrc) return lrc;
        MI355_HIP(hipMemcpyAsync((char *)out + off * S * 8, h->d_out.get(), m * S * 8, hipMemcpyDeviceToHost, st));
        if (freq_out) MI355_HIP(hipMemcpyAsync(freq_out + off * S, h->d_freq.get(), m * S * 4, hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
}
