#!/usr/bin/env python3
"""clFolder probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (R, F, nbin, Ts): (64, 1024, 256, 4096), (16, 4096, 1024, 16384), (64, 1024, 16, 4096), (1, 1024, 128, 2048).  Per shape one
Gaussian float32 filterbank of about --mib MiB (n a multiple of Ts and at least one sub-integration: 4 GiB at the second shape), a model per row of a period of about nbin + 0.37 + r / 8 samples with
a small nudot, hits wanted, no flags, three windows each of
  * the bin-owner route,
  * the generic route (set_generic) on the same handle and buffers, and
  * a device-to-device copy of the input to a buffer of its size: 8 bytes per sample,
ALTERNATING in the same run.  Reported: the time per call, the share of 8 TB/s on 4 bytes per sample plus the output bytes (archive and
hits), the ratio to the copy, and a bound on the share of the bin-owner route's time that finding the rows takes: a fourth timed call
goes through a handle of the same (R, nbin, Ts) with F = 64 on the first 64 / F of the input, whose index launches are the very same
launches and whose fold moves 64 / F of the bytes; that call's time is an upper bound of the index launch's.  The two routes' outputs
are compared bit for bit.  No rate is asserted.
usage: python tools/fold_probe.py [--mib 1024] [--window 0.1] [--no-generic]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

HBM = 8e12
SHAPES = [(64, 1024, 256, 4096), (16, 4096, 1024, 16384), (64, 1024, 16, 4096), (1, 1024, 128, 2048)]


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


def models(R, nbin):
    m = np.empty((R, 3), np.uint64)
    for r in range(R):
        period = nbin + 0.37 + r / 8.0
        m[r] = np.array([int(0.1 * r * 2.0 ** 64) & (2 ** 64 - 1), int(2.0 ** 64 / period), 2 ** 64 - (1 << 16)], dtype=np.uint64)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024, help="input MiB per shape")
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--no-generic", action="store_true", help="leave the generic route out (it takes most of the run)")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clFolder probe: about %d MiB of input per shape, HIP events, windows of >= %.2f s, three windows each, bins / generic / copy "
          "alternating; shares are of %.3g B/s on 4 bytes per sample plus the output bytes" % (a.mib, a.window, HBM))
    for R, F, nbin, Ts in SHAPES:
        m = models(R, nbin)
        blk = pkg.clFolder(*args, R, F, nbin, Ts, m)
        idx = pkg.clFolder(*args, R, 64, nbin, Ts, m)
        ns = max(1, (a.mib << 20) // (4 * R * F * Ts))
        n = ns * Ts
        torch.manual_seed(7)
        d_x = torch.randn(n * R * F, dtype=torch.float32, device="cuda")
        d_c = torch.empty_like(d_x)
        d_y, d_z = (torch.empty(ns * R * nbin * F, dtype=torch.float32, device="cuda") for _ in range(2))
        d_h, d_g = (torch.empty(ns * R * nbin, dtype=torch.int32, device="cuda") for _ in range(2))
        d_xi = d_x[:n * R * 64]
        d_yi = torch.empty(ns * R * nbin * 64, dtype=torch.float32, device="cuda")
        route = blk.route()

        def run_bins():
            blk.set_generic(False)
            blk.set_sample(0)
            blk.work_device(ns, [d_x], [d_y, d_h])

        def run_gen():
            blk.set_generic(True)
            blk.set_sample(0)
            blk.work_device(ns, [d_x], [d_z, d_g])

        def run_index():
            idx.set_sample(0)
            idx.work_device(ns, [d_xi], [d_yi, d_g])

        def run_copy():
            d_c.copy_(d_x)

        run_bins()
        run_index()
        run_copy()
        torch.cuda.synchronize()
        if not a.no_generic:
            run_gen()
            torch.cuda.synchronize()
            if not (torch.equal(d_y.view(torch.int32), d_z.view(torch.int32)) and torch.equal(d_h, d_g)):
                raise SystemExit("(%d, %d, %d, %d): %s and the generic route differ" % (R, F, nbin, Ts, route))
        tb, tg, tc, ti = [], [], [], []
        for _ in range(3):
            tb.append(window(run_bins, a.window))
            if not a.no_generic:
                tg.append(window(run_gen, a.window, cap=2))
            tc.append(window(run_copy, a.window))
            ti.append(window(run_index, a.window))
        nbytes = 4.0 * n * R * F + 4.0 * ns * R * nbin * (F + 1)
        fm = lambda v: " ".join("%9.3f" % (t * 1e3) for t in v)
        print("(R=%d, F=%d, nbin=%d, Ts=%d), %d sub-integrations = %d samples, %.3f GB read + written: %s" % (R, F, nbin, Ts, ns, n, nbytes / 1e9, route))
        print("    bins        %s ms   best %.3f of 8 TB/s; %.2fx the copy's time" % (fm(tb), nbytes / min(tb) / HBM, min(tb) / min(tc)))
        if tg:
            print("    generic     %s ms   best %.5f of 8 TB/s; bins / generic %.5fx of its time%s"
                  % (fm(tg), nbytes / min(tg) / HBM, min(tb) / min(tg), "" if min(tb) <= min(tg) else "  ** the bin-owner route LOSES here **"))
        else:
            print("    generic     not measured")
        print("    copy        %s ms   best %.3f of 8 TB/s on its 8 bytes per sample" % (fm(tc), 8.0 * n * R * F / min(tc) / HBM))
        print("    index+F=64  %s ms   finding the rows takes at most %.3f of the bins route's time" % (fm(ti), min(ti) / min(tb)))
        blk.stop()
        idx.stop()
        del d_x, d_c, d_y, d_z, d_h, d_g, d_xi, d_yi
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
