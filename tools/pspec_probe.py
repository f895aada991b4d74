#!/usr/bin/env python3
"""clPowerSpectrum probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

One 1 GiB complex64 input (2^27 items, four times the 256 MiB Infinity Cache) serves every shape (N, K, H): as many whole spectra as
it holds.  Per shape, three windows each, ALTERNATING in the same run:
  * clPowerSpectrum: Gitems/s of input consumed, and the share of 8 TB/s on the algorithmic traffic 8 (items read) + 4 S N bytes;
  * clFFT alone (same length, no window, no shift) on the same number of frames, contiguous from the start of the same buffer --
    the first stage of the only way to a power spectrum without this block (|X|^2 and the average would still follow), hence a lower
    bound on that way's time.  Where the frames overlap (H < N) there are more frames than the output buffer of clFFT holds: clFFT is
    timed on 2^27 / N frames and its time per frame is used.
The outputs of the first call are compared with a float64 evaluation of the first and the last spectrum (1e-5).
Acceptance: at K >= 16 and H = N the fused route must be faster than clFFT alone (slowest window against fastest); the exit status
says so.  usage: python tools/pspec_probe.py [--log2n 27] [--window 0.2]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS = 8.0
# (N, K, H as a fraction of N, S or None for all that fit)
SHAPES = [(4096, 64, 1.0, None), (4096, 64, 0.5, None), (1024, 16, 1.0, None), (64, 256, 1.0, None), (4096, 1, 1.0, None),
          (4096, None, 1.0, 1), (1000, 64, 1.0, None)]


def window(fn, seconds, cap=4000):
    """seconds per call: events around enough back-to-back calls to fill `seconds` (from one timed call), at least 2"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    reps = int(min(cap, max(2, seconds / max(e0.elapsed_time(e1) / 1e3, 1e-6))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    total = 1 << a.log2n
    print("clPowerSpectrum probe: one input of 2^%d items, HIP events, windows of >= %.2f s, three windows each, alternating with clFFT alone"
          % (a.log2n, a.window))
    d_x = torch.complex(torch.randn(total, device="cuda"), torch.randn(total, device="cuda")).contiguous()
    d_f = torch.empty(total, dtype=torch.complex64, device="cuda")
    bad = []
    for N, K, hf, S in SHAPES:
        H = int(N * hf)
        nframes = (total - N) // H + 1
        if K is None:
            K = nframes // S
        if S is None:
            S = nframes // K
        blk = pkg.clPowerSpectrum(*args, N, K, None, H)
        fft = pkg.clFFT(N, pkg.CLFFT_FORWARD, [], pkg.DTYPE_COMPLEX, *args, 0, 1, False)
        nin, nout = blk.plan(S)
        d_y = torch.full((nout,), float("nan"), dtype=torch.float32, device="cuda")
        nf_fft = min(S * K, total // N)
        run_p = lambda: blk.work_device(S, [d_x], [d_y])                 # noqa: E731
        run_f = lambda: fft.work_device(nf_fft, [d_x], [d_f])            # noqa: E731
        run_p(); run_f()
        torch.cuda.synchronize()
        got = d_y.cpu().numpy().reshape(S, N)
        for s in sorted({0, S - 1}):
            fr = torch.stack([d_x[(s * K + k) * H:(s * K + k) * H + N] for k in range(K)]).to(torch.complex128)
            want = (torch.fft.fft(fr, dim=1).abs() ** 2).sum(dim=0).cpu().numpy() / K
            err = float(np.abs(got[s] - want).max() / want.max())
            if not err <= 1e-5:
                raise SystemExit("(%d, %d, %d) spectrum %d: relerr %.3g" % (N, K, H, s, err))
        tp, tf = [], []
        for _ in range(3):
            tp.append(window(run_p, a.window))
            tf.append(window(run_f, a.window))
        scale_f = S * K / nf_fft  # clFFT's time for as many frames as the spectra hold
        nbytes = 8.0 * nin + 4.0 * nout
        print("(N=%d, K=%d, H=%d, S=%d): %s" % (N, K, H, S, blk.route()))
        print("    clPowerSpectrum %s ms   best %7.2f Gitems/s consumed   %.3f of %.0f TB/s on %.3f GB" %
              (" ".join("%8.3f" % (v * 1e3) for v in tp), S * K * H / min(tp) / 1e9, nbytes / min(tp) / (PEAK_TBS * 1e12), PEAK_TBS, nbytes / 1e9))
        print("    clFFT alone     %s ms   on %d frames%s   %.3f of %.0f TB/s on 16 B per point" %
              (" ".join("%8.3f" % (v * 1e3 * scale_f) for v in tf), nf_fft, "" if scale_f == 1 else " (scaled by %.3f to %d frames)" % (scale_f, S * K),
               16.0 * nf_fft * N / min(tf) / (PEAK_TBS * 1e12), PEAK_TBS))
        print("    clPowerSpectrum / clFFT alone: %.3fx of its time (slowest window against clFFT's fastest: %.3fx)" %
              (min(tp) / (min(tf) * scale_f), max(tp) / (min(tf) * scale_f)))
        if K >= 16 and H == N and blk.route().startswith("fused") and not max(tp) < min(tf) * scale_f:
            bad.append((N, K, H))
        blk.stop(); fft.stop()
        del d_y
    print("fused route faster than clFFT alone at every shape with K >= 16 and H = N: %s" % ("yes" if not bad else "NO: %r" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
