// clBeamformer: tied-array beamformer on the X-engine's int8 frames as gfx950 HIP kernels.  The contract is in include/mi355_clenabled.h;
// the reference module has no beamformer.
//
//     y[t][b][c] = sum_s w[c][b][s] x[t][s][c]          c = (channel f, polarisation p) flattened, complex, exact in int32
//     P[W][b][c] = (float) sum_{t in W} |y[t][b][c]|^2    exact in int64, one conversion
//
// k_bf_mfma   the hot route (F npol a multiple of 8, S <= 256, `in` on 16 bytes).  Per column c the product (beams x stations) . (stations
//             x time) runs on v_mfma_i32_16x16x64_i8 with K = the interleaved (station, {I, Q}) bytes, 32 stations per instruction:
//                 re = [w_re, -w_im] . [I, Q]        im = [w_im, w_re] . [I, Q]
//             so the input bytes are the B operand as they lie in memory and only the weights are folded (a weight is never -128, its
//             negation is a byte).  Two products per complex 16 x 16 x 32 tile: four real multiply-adds per complex one, nothing redundant.
//             A workgroup of 8 waves owns one 16-byte column group (8 columns of a station row), a chunk of BTW beam tiles and a range of
//             units; wave j owns column j and keeps its folded weights -- the stationary operand -- in registers across its time loop.
//             A round covers TT = 8 / KB time tiles of 16 frames: every thread loads the 16-byte pieces of 8 stations of one frame (only
//             pieces inside the frame, and stations < S: the K padding is zeros made in registers), transposes 8 stations x 8 columns of
//             2-byte samples with 32 v_perm_b32 and writes 8 finished B operands to LDS, where the waves read them back with unit stride;
//             the next round's loads are in flight during the products.
//             VOLTAGE: int32 -> float, one 8-byte store per value.  POWER: re^2 + im^2 in int64 per lane over the window, the 16 time
//             lanes meet by shuffles, the 8 columns of the workgroup in LDS (where Stokes I adds the two polarisations), one conversion.
//             A workgroup owns whole windows, so nothing is combined across workgroups: no atomics and no workspace.
// k_bf_gen_*  the generic route: one thread per output, the same integer arithmetic in plain C++.
#include <cstdint>
#include <string>
#include <vector>
#include "common.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int kBfThreads = 512;            // 8 waves: one per column of the workgroup's 16-byte column group
constexpr int kBfMaxS = 512, kBfMaxB = 1024, kBfMaxTi = 4096;
constexpr int kBfMfmaMaxS = 256;           // 8 K blocks of 32 stations
constexpr int kBfTileV4 = 8 * 8 * 64;      // B operands of a round: (TT KB = 8) x 8 columns x 64 lanes, 16 bytes each = 64 KiB
constexpr long long kBfMaxCall = 1ll << 40;

struct BfArgs {
    const unsigned char *in;
    const v4i *tab;     // folded weights in operand order: [c][beam tile][K block][re, im][lane] 16 bytes
    void *out;
    int S, C, F, B, NBT, KBs;  // stations, columns = F npol, channels, beams, beam tiles, K blocks the table holds
    int Tu;             // frames per unit of a workgroup: the window (POWER), the time chunk (VOLTAGE)
    long long T, nW;    // frames of the call, units of Tu frames (the last one may be short in VOLTAGE mode)
    int stokes;
};

__device__ __forceinline__ unsigned bf_perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }

// the column group of a workgroup: with 64 groups or a multiple, the 8 groups that share a 128-byte line are dealt to workgroups that sit
// on the same XCD (consecutive workgroup ids go round the 8 XCDs), so a line is fetched into one L2 and not into eight
__device__ __forceinline__ int bf_group(int id, int ncg)
{
    if (ncg & 63) return id;
    const int x = id & 7, q = id >> 3;
    return (((q >> 3) * 8 + x) << 3) + (q & 7);
}

template <int KB, int BTW, int MODE>
__global__ __launch_bounds__(kBfThreads) void k_bf_mfma(const BfArgs a)
{
    constexpr int TT = 8 / KB;
    extern __shared__ __attribute__((aligned(16))) v4u bf_lds[];
    long long *const pw = (long long *)(bf_lds + kBfTileV4);  // [BTW 16 beams][8 columns]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = bf_group(blockIdx.x, a.C >> 3), bt0 = blockIdx.y * BTW;
    const int c = cg * 8 + wave;
    // the stationary operand
    v4i Are[BTW][KB], Aim[BTW][KB];
#pragma unroll
    for (int bt = 0; bt < BTW; bt++)
#pragma unroll
        for (int kb = 0; kb < KB; kb++) {
            Are[bt][kb] = Aim[bt][kb] = (v4i){0, 0, 0, 0};
            if (bt0 + bt < a.NBT && kb < a.KBs) {
                const v4i *p = a.tab + ((((size_t)c * a.NBT + bt0 + bt) * a.KBs + kb) * 2) * 64 + lane;
                Are[bt][kb] = p[0];
                Aim[bt][kb] = p[64];
            }
        }
    // this thread's piece of a round: frame tt 16 + t16, stations kb 32 + g 8 + 0..7
    const int t16 = tid & 15, g = (tid >> 4) & 3, lkb = (tid >> 6) % KB, ltt = (tid >> 6) / KB;
    const int s0 = lkb * 32 + g * 8;
    const size_t row = (size_t)a.C * 2;
    const int RW = (a.Tu + TT * 16 - 1) / (TT * 16);
    const long long nmy = (a.nW - blockIdx.z + gridDim.z - 1) / gridDim.z;
    const long long nrounds = nmy * RW;
    auto span = [&](long long q, long long &w, long long &tb, long long &te) {
        w = blockIdx.z + (q / RW) * gridDim.z;
        tb = w * a.Tu + (q % RW) * (TT * 16);
        te = (w + 1) * a.Tu;
        if (te > a.T) te = a.T;
    };
    v4u ld[8];
    auto load = [&](long long q) {
        long long w, tb, te;
        span(q, w, tb, te);
        const long long t = tb + ltt * 16 + t16;
        const unsigned char *src = a.in + ((size_t)t * a.S + s0) * row + (size_t)cg * 16;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            ld[r] = (v4u){0u, 0u, 0u, 0u};
            if (t < te && s0 + r < a.S) ld[r] = __builtin_nontemporal_load((const v4u *)(src + (size_t)r * row));
        }
    };
    long long pacc[BTW][4];
#pragma unroll
    for (int bt = 0; bt < BTW; bt++)
#pragma unroll
        for (int r = 0; r < 4; r++) pacc[bt][r] = 0;
    if (nrounds > 0) load(0);
    for (long long q = 0; q < nrounds; q++) {
        long long w, tb, te;
        span(q, w, tb, te);
        __syncthreads();  // the previous round's operands have been read
        // dword d of a piece holds columns 2d, 2d + 1 of one station; operand of column 2d + h: dword e = stations 2e, 2e + 1
#pragma unroll
        for (int d = 0; d < 4; d++) {
            v4u lo, hi;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                lo[e] = bf_perm(ld[2 * e + 1][d], ld[2 * e][d], 0x05040100u);
                hi[e] = bf_perm(ld[2 * e + 1][d], ld[2 * e][d], 0x07060302u);
            }
            bf_lds[((ltt * 8 + 2 * d) * KB + lkb) * 64 + (tid & 63)] = lo;
            bf_lds[((ltt * 8 + 2 * d + 1) * KB + lkb) * 64 + (tid & 63)] = hi;
        }
        __syncthreads();
        if (q + 1 < nrounds) load(q + 1);
#pragma unroll
        for (int tt = 0; tt < TT; tt++) {
            if (tb + tt * 16 >= te) break;  // (uniform)
            v4i re[BTW], im[BTW];
#pragma unroll
            for (int bt = 0; bt < BTW; bt++) re[bt] = im[bt] = (v4i){0, 0, 0, 0};
#pragma unroll
            for (int kb = 0; kb < KB; kb++) {
                const v4u xu = bf_lds[((tt * 8 + wave) * KB + kb) * 64 + lane];
                const v4i X = (v4i){(int)xu[0], (int)xu[1], (int)xu[2], (int)xu[3]};
#pragma unroll
                for (int bt = 0; bt < BTW; bt++) {
                    re[bt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Are[bt][kb], X, re[bt], 0, 0, 0);
                    im[bt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(Aim[bt][kb], X, im[bt], 0, 0, 0);
                }
            }
            // lane: frame = lane & 15, beams (lane >> 4) 4 + 0..3 of every tile
            if (MODE == 0) {
                const long long t = tb + tt * 16 + (lane & 15);
                if (t < te) {
#pragma unroll
                    for (int bt = 0; bt < BTW; bt++)
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            const int b = (bt0 + bt) * 16 + (lane >> 4) * 4 + r;
                            if (b < a.B)
                                __builtin_nontemporal_store((v2f){(float)re[bt][r], (float)im[bt][r]},
                                                            (v2f *)a.out + ((size_t)t * a.B + b) * a.C + c);
                        }
                }
            } else {
                // frames past the window were loaded as zeros and add nothing
#pragma unroll
                for (int bt = 0; bt < BTW; bt++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        pacc[bt][r] += (long long)re[bt][r] * re[bt][r] + (long long)im[bt][r] * im[bt][r];
            }
        }
        if (MODE == 1 && (q % RW) == RW - 1) {  // the window is complete (uniform)
#pragma unroll
            for (int bt = 0; bt < BTW; bt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    long long v = pacc[bt][r];
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
                    if ((lane & 15) == 0) pw[(bt * 16 + (lane >> 4) * 4 + r) * 8 + wave] = v;
                    pacc[bt][r] = 0;
                }
            __syncthreads();  // (the next write of pw is at least two barriers away)
            if (tid < BTW * 128) {
                const int brow = tid >> 3, cc = tid & 7, b = bt0 * 16 + brow;
                if (b < a.B) {
                    float *const o = (float *)a.out;
                    if (a.stokes) {
                        if (!(cc & 1)) o[((size_t)w * a.B + b) * a.F + ((cg * 8 + cc) >> 1)] = (float)(pw[brow * 8 + cc] + pw[brow * 8 + cc + 1]);
                    } else {
                        o[((size_t)w * a.B + b) * a.C + cg * 8 + cc] = (float)pw[brow * 8 + cc];
                    }
                }
            }
        }
    }
}

// generic route: one thread per output.  w: the caller's layout [c][b][s]{re, im}
__global__ __launch_bounds__(256) void k_bf_gen_v(const signed char *__restrict__ in, const signed char *__restrict__ w, float2 *__restrict__ out, int S,
                                                  int C, int B, long long T)
{
    const long long total = T * B * C;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % C), b = (int)((i / C) % B);
        const long long t = i / ((long long)C * B);
        const signed char *x = in + ((size_t)t * S * C + c) * 2, *ww = w + ((size_t)c * B + b) * S * 2;
        int re = 0, im = 0;
        for (int s = 0; s < S; s++) {
            const int xi = x[(size_t)s * C * 2], xq = x[(size_t)s * C * 2 + 1], wr = ww[2 * s], wi = ww[2 * s + 1];
            re += wr * xi - wi * xq;
            im += wr * xq + wi * xi;
        }
        out[i] = make_float2((float)re, (float)im);
    }
}

__global__ __launch_bounds__(256) void k_bf_gen_p(const signed char *__restrict__ in, const signed char *__restrict__ w, float *__restrict__ out, int S,
                                                  int C, int B, int Ti, long long nW, int stokes)
{
    const int CO = stokes ? C / 2 : C, NP = stokes ? 2 : 1;
    const long long total = nW * B * CO;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int co = (int)(i % CO), b = (int)((i / CO) % B);
        const long long W = i / ((long long)CO * B);
        long long sum = 0;
        for (int p = 0; p < NP; p++) {
            const int c = co * NP + p;
            const signed char *ww = w + ((size_t)c * B + b) * S * 2;
            for (int k = 0; k < Ti; k++) {
                const signed char *x = in + ((size_t)(W * Ti + k) * S * C + c) * 2;
                int re = 0, im = 0;
                for (int s = 0; s < S; s++) {
                    const int xi = x[(size_t)s * C * 2], xq = x[(size_t)s * C * 2 + 1], wr = ww[2 * s], wi = ww[2 * s + 1];
                    re += wr * xi - wi * xq;
                    im += wr * xq + wi * xi;
                }
                sum += (long long)re * re + (long long)im * im;
            }
        }
        out[i] = (float)sum;
    }
}

// everything that can be told without a device
int bf_check(int mode, int npol, int S, int F, int B, int Ti, int stokes)
{
    MI355_REQUIRE(mode == MI355_BEAMFORM_VOLTAGE || mode == MI355_BEAMFORM_POWER, "mode must be VOLTAGE (0) or POWER (1)");
    MI355_REQUIRE(npol == 1 || npol == 2, "npol must be 1 or 2");
    MI355_REQUIRE(S >= 1 && S <= kBfMaxS, "num_inputs must be 1 .. 512");
    MI355_REQUIRE(F >= 1, "num_channels must be >= 1");
    MI355_REQUIRE(B >= 1 && B <= kBfMaxB, "num_beams must be 1 .. 1024");
    MI355_REQUIRE(Ti >= 1 && Ti <= kBfMaxTi, "integration must be 1 .. 4096");
    MI355_REQUIRE(mode == MI355_BEAMFORM_POWER || Ti == 1, "integration must be 1 in VOLTAGE mode");
    MI355_REQUIRE(stokes == 0 || stokes == 1, "stokes_i must be 0 or 1");
    MI355_REQUIRE(!stokes || (mode == MI355_BEAMFORM_POWER && npol == 2), "stokes_i needs POWER mode and npol = 2");
    if ((long long)F * npol > (1ll << 31) / (2ll * B * S)) {
        mi355_set_error("clBeamformer: a weight set of 2 x %d x %d x %d x %d bytes is above 2 GiB", F, npol, B, S);
        return MI355_ERR_UNSUPPORTED;
    }
    return MI355_OK;
}

int bf_check_weights(const signed char *w, size_t n)
{
    for (size_t i = 0; i < n; i++) MI355_REQUIRE(w[i] != -128, "a weight component of -128 (the range is -127 .. 127)");
    return MI355_OK;
}

}  // namespace

struct mi355_beamform {
    mi355_ctx *ctx = nullptr;
    int mode = 0, npol = 1, S = 0, F = 0, B = 0, Ti = 1, stokes = 0;
    int C = 0, NBT = 0, KBs = 0, KB = 0, BTW = 0;
    long long frame_bytes = 0, out_unit = 0;
    size_t raw_bytes = 0, raw_pad = 0, tab_bytes = 0;
    bool mfma = false, generic = false;
    std::vector<signed char> w;  // the caller's layout
    mi355_tables tab;            // [raw weights | folded operand table]
    HostPipe pipe;
    std::string route;
    std::mutex lock;
};

namespace {

void bf_name_route(mi355_beamform *h)
{
    char buf[160];
    if (h->mfma && !h->generic)
        snprintf(buf, sizeof buf, "mfma S=%d B=%d F=%d npol=%d kblocks=%d beam_tiles=%d", h->S, h->B, h->F, h->npol, h->KB, h->BTW);
    else snprintf(buf, sizeof buf, "generic S=%d B=%d F=%d npol=%d", h->S, h->B, h->F, h->npol);
    h->route = buf;
}

// a new version from h->w; caller holds the lock (or is create) and has set the device
int bf_upload(mi355_beamform *h)
{
    std::vector<signed char> img(h->raw_pad + h->tab_bytes, 0);
    memcpy(img.data(), h->w.data(), h->raw_bytes);
    if (h->mfma) {
        signed char *tab = img.data() + h->raw_pad;
        for (int c = 0; c < h->C; c++)
            for (int b = 0; b < h->B; b++) {
                const signed char *src = h->w.data() + ((size_t)c * h->B + b) * h->S * 2;
                const int bt = b >> 4, r = b & 15;
                for (int s = 0; s < h->S; s++) {
                    const int kb = s >> 5, g = (s >> 3) & 3, j = s & 7;
                    signed char *op = tab + (((((size_t)c * h->NBT + bt) * h->KBs + kb) * 2) * 64 + (g * 16 + r)) * 16 + 2 * j;
                    const signed char wr = src[2 * s], wi = src[2 * s + 1];
                    op[0] = wr; op[1] = (signed char)-wi;        // re = w_re I - w_im Q
                    op[1024] = wi; op[1025] = wr;                // im = w_im I + w_re Q
                }
            }
    }
    return h->tab.publish(h->ctx, img.data(), img.size(), "mi355_beamform: weight");
}

template <int KB, int BTW>
int bf_launch_mfma(mi355_beamform *h, const BfArgs &a, dim3 grid, hipStream_t st)
{
    const size_t lds = (size_t)kBfTileV4 * 16 + (size_t)BTW * 16 * 8 * 8;
    if (h->mode == MI355_BEAMFORM_VOLTAGE) {
        MI355_HIP(hipFuncSetAttribute((const void *)k_bf_mfma<KB, BTW, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_bf_mfma<KB, BTW, 0>), grid, dim3(kBfThreads), lds, st, a);
    } else {
        MI355_HIP(hipFuncSetAttribute((const void *)k_bf_mfma<KB, BTW, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_bf_mfma<KB, BTW, 1>), grid, dim3(kBfThreads), lds, st, a);
    }
    MI355_HIP(hipGetLastError());
    return MI355_OK;
}

// caller holds the lock and has set the device
int bf_launch(mi355_beamform *h, long long nunits, const void *in, void *out, hipStream_t st)
{
    const int cus = mi355_cus(h->ctx);
    const long long T = nunits * h->Ti;
    const signed char *d_raw = (const signed char *)h->tab.current();
    int rc = MI355_OK;
    if (h->mfma && !h->generic && (reinterpret_cast<uintptr_t>(in) & 15u) == 0) {
        BfArgs a = {};
        a.in = (const unsigned char *)in;
        a.tab = (const v4i *)(d_raw + h->raw_pad);
        a.out = out;
        a.S = h->S; a.C = h->C; a.F = h->F; a.B = h->B; a.NBT = h->NBT; a.KBs = h->KBs;
        a.T = T; a.stokes = h->stokes;
        const int ncg = h->C / 8, nchunk = (h->NBT + h->BTW - 1) / h->BTW;
        const long long xy = (long long)ncg * nchunk;
        long long want = (2ll * cus + xy - 1) / xy;  // workgroups along time / windows for two rounds of the device
        if (want > 65535) want = 65535;
        if (h->mode == MI355_BEAMFORM_VOLTAGE) {
            const int round = (8 / h->KB) * 16;
            long long tu = (T + want - 1) / want;
            tu = (tu + round - 1) / round * round;
            if (tu > (1 << 20)) tu = 1 << 20;
            a.Tu = (int)tu;
            a.nW = (T + tu - 1) / tu;
        } else {
            a.Tu = h->Ti;
            a.nW = nunits;
        }
        const dim3 grid((unsigned)ncg, (unsigned)nchunk, (unsigned)(a.nW < want ? a.nW : want));
        switch (h->KB) {
        case 1: rc = bf_launch_mfma<1, 4>(h, a, grid, st); break;
        case 2: rc = bf_launch_mfma<2, 4>(h, a, grid, st); break;
        case 4: rc = bf_launch_mfma<4, 2>(h, a, grid, st); break;
        default: rc = bf_launch_mfma<8, 1>(h, a, grid, st); break;
        }
    } else {
        const long long total = h->mode == MI355_BEAMFORM_VOLTAGE ? T * h->B * h->C : nunits * h->B * (h->stokes ? h->F : h->C);
        const long long blocks = (total + 255) / 256, cap = (long long)cus * 32;
        const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
        if (h->mode == MI355_BEAMFORM_VOLTAGE)
            hipLaunchKernelGGL(k_bf_gen_v, grid, dim3(256), 0, st, (const signed char *)in, d_raw, (float2 *)out, h->S, h->C, h->B, T);
        else
            hipLaunchKernelGGL(k_bf_gen_p, grid, dim3(256), 0, st, (const signed char *)in, d_raw, (float *)out, h->S, h->C, h->B, h->Ti, nunits,
                               h->stokes);
        MI355_HIP(hipGetLastError());
    }
    if (rc) return rc;
    return h->tab.used(st);  // this version may be released behind this launch
}

int bf_args(const mi355_beamform *h, long long nunits, const void *in, const void *out)
{
    MI355_REQUIRE(nunits >= 0, "nunits is negative");
    if (nunits == 0) return MI355_OK;
    MI355_REQUIRE(in && out, "NULL buffer");
    MI355_REQUIRE((reinterpret_cast<uintptr_t>(in) & 1u) == 0, "in must be 2-byte aligned");
    if (h->mode == MI355_BEAMFORM_VOLTAGE) MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, "out must be 8-byte aligned");
    else MI355_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0, "out must be 4-byte aligned");
    const long long unit_in = h->frame_bytes * h->Ti;
    if (nunits > kBfMaxCall / unit_in) {
        mi355_set_error("clBeamformer: %lld units of %lld input bytes in one call (the limit is 2^40 bytes)", nunits, unit_in);
        return MI355_ERR_UNSUPPORTED;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    MI355_REQUIRE(!(a < b + (uintptr_t)(nunits * h->out_unit) && b < a + (uintptr_t)(nunits * unit_in)),
                  "clBeamformer does not work in place: in and out overlap");
    return MI355_OK;
}

}  // namespace

extern "C" int mi355_beamform_plan(int mode, int npol, int num_inputs, int num_channels, int num_beams, int integration, int stokes_i,
                                   long long *frame_bytes, int *frames_per_unit, long long *out_bytes_per_unit)
{
    if (frame_bytes) *frame_bytes = 0;
    if (frames_per_unit) *frames_per_unit = 0;
    if (out_bytes_per_unit) *out_bytes_per_unit = 0;
    const int rc = bf_check(mode, npol, num_inputs, num_channels, num_beams, integration, stokes_i);
    if (rc) return rc;
    if (frame_bytes) *frame_bytes = 2ll * num_inputs * num_channels * npol;
    if (frames_per_unit) *frames_per_unit = integration;
    if (out_bytes_per_unit)
        *out_bytes_per_unit = mode == MI355_BEAMFORM_VOLTAGE ? 8ll * num_beams * num_channels * npol
                                                              : 4ll * num_beams * num_channels * (stokes_i ? 1 : npol);
    return MI355_OK;
}

extern "C" int mi355_beamform_create(mi355_ctx *ctx, int mode, int npol, int num_inputs, int num_channels, int num_beams, int integration,
                                     int stokes_i, const void *weights, mi355_beamform **out)
{
    MI355_REQUIRE(out != nullptr, "NULL argument");
    *out = nullptr;
    // everything that can be told without a device comes first
    long long fb = 0, ou = 0;
    int rc = mi355_beamform_plan(mode, npol, num_inputs, num_channels, num_beams, integration, stokes_i, &fb, nullptr, &ou);
    if (rc) return rc;
    const size_t nw = (size_t)2 * num_channels * npol * num_beams * num_inputs;
    if (weights) {
        rc = bf_check_weights((const signed char *)weights, nw);
        if (rc) return rc;
    }
    MI355_REQUIRE(ctx != nullptr, "NULL context");
    mi355_beamform *h = new (std::nothrow) mi355_beamform();
    if (!h) return MI355_ERR_NOMEM;
    h->ctx = ctx; h->mode = mode; h->npol = npol; h->S = num_inputs; h->F = num_channels; h->B = num_beams; h->Ti = integration;
    h->stokes = stokes_i; h->C = num_channels * npol; h->frame_bytes = fb; h->out_unit = ou;
    h->NBT = (h->B + 15) / 16;
    h->KBs = (h->S + 31) / 32;
    h->mfma = h->C % 8 == 0 && h->S <= kBfMfmaMaxS;
    h->KB = h->KBs <= 1 ? 1 : (h->KBs <= 2 ? 2 : (h->KBs <= 4 ? 4 : 8));
    h->BTW = h->KB <= 2 ? 4 : 8 / h->KB;
    h->raw_bytes = nw;
    h->raw_pad = (nw + 255) & ~(size_t)255;
    h->tab_bytes = h->mfma ? (size_t)h->C * h->NBT * h->KBs * 2 * 1024 : 0;
    if (weights) h->w.assign((const signed char *)weights, (const signed char *)weights + nw);
    else h->w.assign(nw, 0);
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        mi355_set_error("mi355_beamform_create: %s", hipGetErrorString(e));
        rc = MI355_ERR_HIP;
    } else {
        rc = bf_upload(h);
        if (rc == MI355_OK) rc = h->pipe.init(ctx);
    }
    if (rc) { mi355_beamform_destroy(h); return rc; }
    bf_name_route(h);
    mi355_log(ctx, MI355_LOG_INFO, "clBeamformer: %s, %d inputs, %d channels, %d pol, %d beams, integration %d%s: %s",
              mode == MI355_BEAMFORM_POWER ? "power" : "voltage", h->S, h->F, h->npol, h->B, h->Ti, h->stokes ? ", Stokes I" : "", h->route.c_str());
    *out = h;
    return MI355_OK;
}

extern "C" int mi355_beamform_destroy(mi355_beamform *h)
{
    if (!h) return MI355_OK;
    (void)hipSetDevice(h->ctx->device);
    h->tab.release();
    h->pipe.release();
    delete h;
    return MI355_OK;
}

extern "C" int mi355_beamform_set_weights(mi355_beamform *h, const void *weights)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(weights != nullptr, "weights is NULL");
    const int rc = bf_check_weights((const signed char *)weights, h->raw_bytes);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const std::vector<signed char> old = h->w;
    h->w.assign((const signed char *)weights, (const signed char *)weights + h->raw_bytes);
    const int rc2 = bf_upload(h);
    if (rc2) h->w = old;  // the version in use is still the old one
    return rc2;
}

extern "C" int mi355_beamform_set_beam_weights(mi355_beamform *h, int beam, const void *w_beam)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    MI355_REQUIRE(w_beam != nullptr, "w_beam is NULL");
    MI355_REQUIRE(beam >= 0 && beam < h->B, "beam out of range");
    const size_t per = (size_t)2 * h->S;
    const int rc = bf_check_weights((const signed char *)w_beam, per * h->C);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    const std::vector<signed char> old = h->w;
    for (int c = 0; c < h->C; c++) memcpy(h->w.data() + ((size_t)c * h->B + beam) * per, (const signed char *)w_beam + (size_t)c * per, per);
    const int rc2 = bf_upload(h);
    if (rc2) h->w = old;
    return rc2;
}

extern "C" int mi355_beamform_get_weights(const mi355_beamform *h, void *out, long long cap_bytes)
{
    MI355_REQUIRE(h && out, "NULL argument");
    std::lock_guard<std::mutex> g(const_cast<mi355_beamform *>(h)->lock);
    MI355_REQUIRE(cap_bytes >= (long long)h->raw_bytes, "out too small");
    memcpy(out, h->w.data(), h->raw_bytes);
    return MI355_OK;
}

extern "C" int mi355_beamform_num_beams(const mi355_beamform *h) { return h ? h->B : MI355_ERR_INVALID_ARG; }
extern "C" long long mi355_beamform_frame_bytes(const mi355_beamform *h) { return h ? h->frame_bytes : MI355_ERR_INVALID_ARG; }
extern "C" long long mi355_beamform_out_bytes_per_unit(const mi355_beamform *h) { return h ? h->out_unit : MI355_ERR_INVALID_ARG; }

extern "C" int mi355_beamform_set_generic(mi355_beamform *h, int on)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    std::lock_guard<std::mutex> g(h->lock);
    h->generic = on != 0;
    bf_name_route(h);
    return MI355_OK;
}

extern "C" const char *mi355_beamform_route(const mi355_beamform *h) { return h ? h->route.c_str() : ""; }

extern "C" int mi355_beamform_work_dev(mi355_beamform *h, long long nunits, const void *in, void *out, void *stream)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    const int rc = bf_args(h, nunits, in, out);
    if (rc || nunits == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    return bf_launch(h, nunits, in, out, mi355_pick_stream(h->ctx, stream));
}

extern "C" int mi355_beamform_work(mi355_beamform *h, long long nunits, const void *in, void *out)
{
    MI355_REQUIRE(h != nullptr, "handle is NULL");
    int rc = bf_args(h, nunits, in, out);
    if (rc || nunits == 0) return rc;
    std::lock_guard<std::mutex> g(h->lock);
    std::lock_guard<std::mutex> gc(h->ctx->lock);
    MI355_HIP(hipSetDevice(h->ctx->device));
    // pieces of whole units sized from the input, at least one unit; one staging slot: the pieces run one after the other
    const size_t unit_in = (size_t)h->frame_bytes * h->Ti, unit_out = (size_t)h->out_unit;
    const size_t bigger = unit_in > unit_out ? unit_in : unit_out;
    size_t piece = mi355_chunk_bytes((size_t)nunits * bigger, h->ctx) / bigger;
    if (piece < 1) piece = 1;
    if (piece > (size_t)nunits) piece = (size_t)nunits;
    const size_t in_cap = piece * unit_in;
    rc = h->pipe.ensure(1, &in_cap, piece * unit_out, 1);
    if (rc) return rc;
    const HostPipe::Plan plan{1, true, false};  // one slot, stream[0], never direct
    auto units = [&](size_t ci) { return HostPipe::part((size_t)nunits, piece, ci); };
    return h->pipe.run(
        ((size_t)nunits + piece - 1) / piece, plan,
        [&](size_t ci) {
            return HostPipe::Chunk{{(const char *)in + ci * piece * unit_in}, {units(ci) * unit_in}, (char *)out + ci * piece * unit_out, units(ci) * unit_out};
        },
        [&](size_t ci, void *const *d_in, void *d_out, hipStream_t st) { return bf_launch(h, (long long)units(ci), d_in[0], d_out, st); });
}
