// clPolyphaseSynthesizer: the per-phase FIR over transformed frames that sit in an LDS ring, shared by the power-of-two kernel
// (synth.hip) and the mixed-radix one (fft_mr.hip).
//
// The ring is `nreg` regions of `rs` slots; a region holds the F frames of one tile, value r of frame e at PAD::at(e M + r).  The
// tile being filtered is region `reg`, the tile before it region reg - 1 (mod nreg) and so on: (nreg - 1) F >= T - 1 older frames.
// A thread owns phase r of JB consecutive frames: one fmaf chain per output and component, p ascending from +0,
//     y[e][r] = sum_p tp[p M + r] V[e - p][r]
// with a window of JB transformed values in registers that slides one frame down per tap -- one 8-byte LDS read and one tap read
// serve JB outputs.  Lanes run along r, so a wave reads consecutive slots and stores consecutive outputs.
#pragma once
#include <hip/hip_runtime.h>

namespace synthf {

typedef float v2f __attribute__((ext_vector_type(2)));

struct PadNone { __device__ static __forceinline__ int at(int i) { return i; } };
struct Pad32 { __device__ static __forceinline__ int at(int i) { return i + (i >> 5); } };  // fft_mr.hip's slot()

struct FirArgs {
    int M, T, F, nreg, rs;
    unsigned m_M;  // ceil(2^32 / M), M >= 2: exact quotients below 2^16
};

// out_tile: output of the tile's frame 0; nvalid: frames of the tile that exist (the rest is neither computed nor stored)
template <class PAD, int JB, class C>
__device__ __forceinline__ void fir_tile(const C *ring, const FirArgs &f, int reg, const float *tp, v2f *out_tile, int nvalid, int tid, int th)
{
    const int nblk = (f.F + JB - 1) / JB, items = nblk * f.M;
    for (int idx = tid; idx < items; idx += th) {
        const int jb = (int)__umulhi((unsigned)idx, f.m_M), r = idx - jb * f.M, e0 = jb * JB;
        if (e0 >= nvalid) continue;
        float ax[JB], ay[JB];
        C w[JB];
#pragma unroll
        for (int j = 0; j < JB; j++) {
            ax[j] = 0.f;
            ay[j] = 0.f;
            const int e = e0 + j < f.F ? e0 + j : f.F - 1;  // (past the tile: a value that is dropped below)
            w[j] = ring[reg * f.rs + PAD::at(e * f.M + r)];
        }
        int rg = reg, e = e0;
        const float *t = tp + r;
        for (int p = 0; p < f.T; p++) {
            const float g = t[(size_t)p * f.M];
#pragma unroll
            for (int j = 0; j < JB; j++) {
                ax[j] = fmaf(g, w[j].x, ax[j]);
                ay[j] = fmaf(g, w[j].y, ay[j]);
            }
            if (p + 1 < f.T) {
#pragma unroll
                for (int j = JB - 1; j > 0; j--) w[j] = w[j - 1];
                if (--e < 0) {
                    e = f.F - 1;
                    rg = rg ? rg - 1 : f.nreg - 1;
                }
                w[0] = ring[rg * f.rs + PAD::at(e * f.M + r)];
            }
        }
#pragma unroll
        for (int j = 0; j < JB; j++)
            if (e0 + j < nvalid) __builtin_nontemporal_store((v2f){ax[j], ay[j]}, out_tile + (size_t)(e0 + j) * f.M + r);
    }
}

}  // namespace synthf
