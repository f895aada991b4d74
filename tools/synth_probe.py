#!/usr/bin/env python3
"""clPolyphaseSynthesizer probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

For every probe shape (M, T, map), about 2^26 outputs per call (input and output together pass the 256 MiB Infinity Cache):
  * GS/s of output and the share of 8 TB/s on the algorithmic traffic, 8 (nmap + M) bytes per frame, for the route the library
    picks (fused pow2 / fused mixed-radix);
  * the generic route on the same shape (a handle made with MI355_SYNTH_GENERIC=1), ALTERNATING with the fused one in the same
    run, three windows each.  The generic route transforms with M products per value, so at 1024 channels and more it is timed
    on 2^22 outputs and compared by rate;
  * the two routes' outputs compared (tolerance 1e-5; between routes the bits may differ);
  * for the power-of-two kernel, identity map: the same kernel with its taps read through the caches instead of from LDS
    (MI355_SYNTH_TAPS_GLOBAL=1), bit-identical outputs required.
Every handle's route() must be the one the row claims.  The last lines say where the fused form beats the generic one by more
than the 4 % box spread; a shape where it does not should be routed to generic.
usage: python tools/synth_probe.py [--log2n 26] [--window 0.2]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS = 8.0
SHAPES = [(64, 32, "ident"), (64, 32, "half"), (16, 8, "ident"), (256, 16, "ident"), (1024, 8, "ident"), (4096, 4, "ident"),
          (100, 8, "ident"), (12, 16, "ident")]
GENERIC_LOG2N_LARGE_M = 22


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


def made(pkg, args, g, M, m, generic):
    os.environ.pop("MI355_SYNTH_GENERIC", None)
    if generic:
        os.environ["MI355_SYNTH_GENERIC"] = "1"  # read when the handle is created
    try:
        blk = pkg.clPolyphaseSynthesizer(*args, g, M, m)
    finally:
        os.environ.pop("MI355_SYNTH_GENERIC", None)
    if (blk.route() == "generic") != generic:
        raise SystemExit("M=%d: asked for the %s route, got '%s'" % (M, "generic" if generic else "fused", blk.route()))
    return blk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clPolyphaseSynthesizer probe: about 2^%d outputs per call, HIP events, windows of >= %.2f s, three windows each, alternating" %
          (a.log2n, a.window))
    verdicts = []
    for M, T, kind in SHAPES:
        m = None if kind == "ident" else np.random.default_rng(M).permutation(M)[:M // 2].astype(np.int32)
        nmap = M if m is None else int(m.size)
        k = np.arange(T * M) - (T * M - 1) / 2.0
        g = (np.sinc(k / M) * np.hamming(T * M)).astype(np.float32)  # a windowed-sinc prototype at 1 / M
        fused, gen = made(pkg, args, g, M, m, False), made(pkg, args, g, M, m, True)
        nf = (1 << a.log2n) // M
        nf_gen = nf if M < 1024 else min(nf, (1 << GENERIC_LOG2N_LARGE_M) // M)
        n_in = fused.plan(nf)[0]
        d_x = torch.complex(torch.randn(n_in, device="cuda"), torch.randn(n_in, device="cuda")).contiguous()
        d_y = torch.empty(nf * M, dtype=torch.complex64, device="cuda")
        d_z = torch.empty(nf_gen * M, dtype=torch.complex64, device="cuda")
        run_f = lambda: fused.work_device(nf, [d_x], [d_y])      # noqa: E731
        run_g = lambda: gen.work_device(nf_gen, [d_x], [d_z])    # noqa: E731
        run_f(); run_g()  # warm-up of both, and the two routes compute the same thing
        torch.cuda.synchronize()
        diff = float((d_y[:nf_gen * M] - d_z).abs().max()) / float(d_z.abs().max())
        if not diff < 1e-5:
            raise SystemExit("(%d, %d, %s): fused and generic disagree, max rel diff %.3g" % (M, T, kind, diff))
        tf, tg = [], []
        for _ in range(3):
            tf.append(window(run_f, a.window))
            tg.append(window(run_g, a.window, cap=50))
        rate_f, rate_g = nf * M / min(tf), nf_gen * M / min(tg)
        worst_f, best_g = nf * M / max(tf), rate_g
        share = 8.0 * (nmap + M) * nf / min(tf) / (PEAK_TBS * 1e12)
        print("(M=%4d, T=%2d, %s map, nmap=%d): %s" % (M, T, kind, nmap, fused.route()))
        print("    fused    %s ms   best %7.1f GS/s of output   %.3f of %.0f TB/s on %.2f GB" %
              (" ".join("%8.3f" % (v * 1e3) for v in tf), rate_f / 1e9, share, PEAK_TBS, 8.0 * (nmap + M) * nf / 1e9))
        print("    generic  %s ms   best %7.1f GS/s of output on %d frames   (max rel diff to fused %.2g)" %
              (" ".join("%8.3f" % (v * 1e3) for v in tg), rate_g / 1e9, nf_gen, diff))
        print("    fused / generic: %.1fx faster (slowest fused window against the fastest generic one: %.2fx)" % (rate_f / rate_g, worst_f / best_g))
        verdicts.append(((M, T, kind), worst_f > 1.04 * best_g))
        if fused.route().startswith("fused pow2") and kind == "ident":
            # the same kernel with its taps read through the caches instead of from LDS (where they fit the LDS at all): same bits
            os.environ["MI355_SYNTH_TAPS_GLOBAL"] = "1"
            try:
                alt = made(pkg, args, g, M, m, False)
            finally:
                os.environ.pop("MI355_SYNTH_TAPS_GLOBAL", None)
            want = d_y.clone()
            run_a = lambda: alt.work_device(nf, [d_x], [d_y])  # noqa: E731
            run_a()
            torch.cuda.synchronize()
            same = bool(torch.equal(want.view(torch.int32), d_y.view(torch.int32)))
            ta = [window(run_a, a.window) for _ in range(3)]
            print("    taps through the caches: %s ms   best %7.1f GS/s   (outputs %s those with the taps in LDS)" %
                  (" ".join("%8.3f" % (v * 1e3) for v in ta), nf * M / min(ta) / 1e9, "bit-identical to" if same else "DIFFER from"))
            alt.stop()
            del want
        fused.stop(); gen.stop()
        del d_x, d_y, d_z
        torch.cuda.empty_cache()
    bad = [s for s, ok in verdicts if not ok]
    print("fused beats generic by more than the 4 %% box spread at every shape: %s" % ("yes" if not bad else "NO: %r" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
