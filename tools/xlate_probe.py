#!/usr/bin/env python3
"""clFreqXlatingFIRFilter probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

One 2 GiB complex64 input (2^28 items, eight times the 256 MiB Infinity Cache) serves every shape (D, K, C).  Per shape, three windows
each, ALTERNATING in the same run:
  * the fused route (k_xlate): Gitems/s of input, the share of 8 TB/s on the algorithmic traffic 8 (n_in + C n_out) bytes, and the
    fp32 rate on 8 K C flops per output (4 K C fused multiply-adds) against the 157.3 TFLOPS vector peak (78.6 without packed FMAs);
  * the generic route on the same handle (set_generic: per channel clComplexFilter + the rotate kernel);
  * the only way that existed before the block: per channel clComplexFilter with the same band-pass taps and decimation, clSignalSource
    at the decimated rate and clMultiply (three launches and two extra round trips of the decimated stream per channel).
The first call of every route is compared with the fused route's output (1e-4 of the largest magnitude; the composition's NCO is a
float recurrence).  No rate is asserted.  usage: python tools/xlate_probe.py [--log2n 28] [--window 0.1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS = 8.0
PEAK_TFLOPS = 157.3
SHAPES = [(16, 65, 1), (16, 65, 8), (8, 129, 4), (64, 257, 16), (25, 101, 3), (2, 33, 2)]
FS = 1.0e6


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    total = 1 << a.log2n
    print("clFreqXlatingFIRFilter probe: one input of 2^%d items, HIP events, windows of >= %.2f s, three windows each, fused / generic / "
          "clComplexFilter + clSignalSource + clMultiply alternating" % (a.log2n, a.window))
    d_x = torch.complex(torch.randn(total, device="cuda"), torch.randn(total, device="cuda")).contiguous()
    rng = np.random.default_rng(5)
    for D, K, C in SHAPES:
        n = (total - (K - 1)) // D
        h = (rng.standard_normal(K) / np.sqrt(K)).astype(np.float32)
        freqs = [(c + 0.37) * FS / (2.0 * C) - FS / 4 for c in range(C)]
        blk = pkg.clFreqXlatingFIRFilter(*args, D, h, freqs, FS, True)
        fused_route = blk.route()
        outs = [torch.full((n,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(C)]
        chk = [torch.empty(n, dtype=torch.complex64, device="cuda") for _ in range(C)]
        # the composition: the same band-pass taps, an NCO at -f_c at the decimated rate, a multiply
        filt = [pkg.clComplexFilter(*args, D, blk.bandpass_taps(c), 1, 0, True) for c in range(C)]
        nco = [pkg.clSignalSource(pkg.DTYPE_COMPLEX, *args, FS / D, 1, -freqs[c], 1.0) for c in range(C)]
        mul = pkg.clMathOp(pkg.DTYPE_COMPLEX, *args, pkg.MATHOP_MULTIPLY)
        tmp = torch.empty(n, dtype=torch.complex64, device="cuda")
        car = torch.empty(n, dtype=torch.complex64, device="cuda")

        def reset():
            for c in range(C):
                blk.set_phase(0, c)
                nco[c].set_phase(0.0)

        def run_fused():
            blk.work_device(n, [d_x], outs)

        def run_old(dst=None):
            for c in range(C):
                filt[c].work_device(n, [d_x], [tmp])
                nco[c].work_device(n, [], [car])
                mul.work_device(n, [tmp, car], [(dst or outs)[c]])

        reset()
        run_fused()
        torch.cuda.synchronize()
        want = [o.clone() for o in outs]
        scale = max(float(w.abs().max()) for w in want)
        assert all(bool(torch.isfinite(torch.view_as_real(w)).all()) for w in want), "fused route left an output unwritten"
        blk.set_generic(True)
        generic_route = blk.route()
        reset()
        blk.work_device(n, [d_x], chk)
        e_gen = max(float((g - w).abs().max()) for g, w in zip(chk, want)) / scale
        reset()
        run_old(chk)
        torch.cuda.synchronize()
        e_old = max(float((g - w).abs().max()) for g, w in zip(chk, want)) / scale
        if not (e_gen <= 1e-4 and e_old <= 1e-4):
            raise SystemExit("(%d, %d, %d): generic differs from fused by %.3g, the composition by %.3g of the largest magnitude" % (D, K, C, e_gen, e_old))
        tf, tg, to = [], [], []
        for _ in range(3):
            blk.set_generic(False)
            tf.append(window(run_fused, a.window))
            blk.set_generic(True)
            tg.append(window(run_fused, a.window))
            to.append(window(run_old, a.window))
        nin = n * D + K - 1
        nbytes = 8.0 * (nin + C * n)
        flops = 8.0 * K * C * n
        print("(D=%d, K=%d, C=%d), %d outputs per channel: %s" % (D, K, C, n, fused_route))
        for name, t in (("fused", tf), (generic_route.split(" ")[0], tg), ("filter+nco+multiply", to)):
            print("    %-20s %s ms   best %7.2f Gitems/s of input   %.3f of %.0f TB/s on %.3f GB   %6.2f TFLOPS = %.3f of %.1f" %
                  (name, " ".join("%8.3f" % (v * 1e3) for v in t), nin / min(t) / 1e9, nbytes / min(t) / (PEAK_TBS * 1e12), PEAK_TBS, nbytes / 1e9,
                   flops / min(t) / 1e12, flops / min(t) / 1e12 / PEAK_TFLOPS, PEAK_TFLOPS))
        print("    fused / generic %.3fx of its time, fused / composition %.3fx of its time (%.2fx faster); generic and composition within %.2g / %.2g of fused" %
              (min(tf) / min(tg), min(tf) / min(to), min(to) / min(tf), e_gen, e_old))
        for b in [blk, mul] + filt + nco:
            b.stop()
        del outs, chk, tmp, car, want
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
