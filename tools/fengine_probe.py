#!/usr/bin/env python3
"""clFEngine probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (S, npol, F, P): (64, 2, 1024, 1), (64, 2, 1024, 4), (64, 2, 4096, 8), (16, 1, 64, 4) on the fused route and (64, 2, 1000, 4) on
the generic route.  Per shape R = S npol complex64 streams of together `--mib` MiB, Gaussian, gains for an rms of 30 per output
component; three windows each, ALTERNATING in the same run:
  * clFEngine on its own route: the time per call, Gitems/s consumed, and the share of 8 TB/s on 8 (items read) + 2 (items written) bytes;
  * clFFT alone on the same R n frames (complex64 in, complex64 out: 16 bytes per item) -- the first stage of the only way to these
    frames before the block existed.
The first frames of every fused shape are compared with the generic route on the same handle: a component may differ by one where its
value lies at a rounding boundary; the count is printed, and anything else is an error.  No rate is asserted.
usage: python tools/fengine_probe.py [--mib 1024] [--window 0.1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS = 8.0
SHAPES = [(64, 2, 1024, 1), (64, 2, 1024, 4), (64, 2, 4096, 8), (16, 1, 64, 4), (64, 2, 1000, 4)]


def window(fn, seconds, cap=2000):
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


def taps(F, P):
    n = np.arange(P * F)
    return (np.sinc((n - (P * F - 1) / 2.0) / F) * np.hamming(P * F)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clFEngine probe: complex64 inputs of together %d MiB, HIP events, windows of >= %.2f s, three windows each, clFEngine / clFFT "
          "alternating" % (a.mib, a.window))
    for S, npol, F, P in SHAPES:
        R = S * npol
        n = max(1, ((a.mib << 20) // (8 * R * F)) - (P - 1))  # frames per call
        items = (n + P - 1) * F
        h = taps(F, P)
        # Gaussian streams of unit variance per component: a component of X[f] has the variance sum(h^2)
        gain = np.full((R, F), 30.0 / np.sqrt(float((h.astype(np.float64) ** 2).sum())), np.float32)
        blk = pkg.clFEngine(*args, npol, S, F, h, P, True, gain)
        d_all = torch.randn((R, items, 2), dtype=torch.float32, device="cuda")
        d_x = [torch.view_as_complex(d_all[r]) for r in range(R)]
        d_y = torch.full((n * blk.frame_bytes(),), -128, dtype=torch.int8, device="cuda")
        route = blk.route()

        def run_fe():
            blk.work_device(n, d_x, [d_y])

        run_fe()
        torch.cuda.synchronize()
        assert not bool((d_y == -128).any()), "an output byte was left unwritten"
        rms = float(d_y.float().std())
        clip_share = float(blk.clips(reset=True).sum()) / d_y.numel()
        note = ""
        if route.startswith("fused"):
            m = min(n, 2 * (4096 // F) + 1)
            first = d_y[:m * blk.frame_bytes()].clone()
            blk.set_generic(True)
            chk = torch.empty_like(first)
            blk.work_device(m, d_x, [chk])
            torch.cuda.synchronize()
            blk.set_generic(False)
            blk.clips(reset=True)
            diff = (first.to(torch.int16) - chk.to(torch.int16)).abs()
            if int(diff.max()) > 1:
                raise SystemExit("(%d, %d, %d, %d): %s and the generic route differ by more than one" % (S, npol, F, P, route))
            note = "; %d of %d components of the first %d frames differ by one from the generic route" % (int((diff != 0).sum()), diff.numel(), m)
        fft = pkg.clFFT(F, pkg.CLFFT_FORWARD, [], pkg.DTYPE_COMPLEX, *args)
        nfr = R * n
        d_fi = d_all.reshape(-1)[:nfr * F * 2]
        d_fo = torch.empty(nfr * F * 2, dtype=torch.float32, device="cuda")

        def run_fft():
            fft.work_device(nfr, [d_fi], [d_fo])

        run_fft()
        torch.cuda.synchronize()
        tf, tx = [], []
        for _ in range(3):
            tf.append(window(run_fe, a.window))
            tx.append(window(run_fft, a.window))
        blk.clips(reset=True)
        nbytes = 8.0 * R * items + 2.0 * R * n * F
        print("(S=%d, npol=%d, F=%d, P=%d), %d frames per call: %s (output rms %.1f, clipped %.4f %%%s)" % (S, npol, F, P, n, route, rms, 100 * clip_share, note))
        print("    clFEngine  %s ms   best %8.1f Gitems/s   %.3f of %.0f TB/s on %.3f GB (read %.3f + written %.3f)" %
              (" ".join("%8.3f" % (v * 1e3) for v in tf), R * n * F / min(tf) / 1e9, nbytes / min(tf) / (PEAK_TBS * 1e12), PEAK_TBS, nbytes / 1e9,
               8.0 * R * items / 1e9, 2.0 * R * n * F / 1e9))
        print("    clFFT      %s ms   best %8.1f Gitems/s   %.3f of %.0f TB/s on %.3f GB; clFEngine / clFFT %.3fx of its time" %
              (" ".join("%8.3f" % (v * 1e3) for v in tx), nfr * F / min(tx) / 1e9, 16.0 * nfr * F / min(tx) / (PEAK_TBS * 1e12), PEAK_TBS,
               16.0 * nfr * F / 1e9, min(tf) / min(tx)))
        blk.stop()
        fft.stop()
        del d_all, d_x, d_y, d_fi, d_fo
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
