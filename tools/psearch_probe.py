#!/usr/bin/env python3
"""clPulseSearch probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (R, D, K, Tb, order): (64, 1024, 10, 1024) in both orders, (16, 512, 13, 4096) TRIAL_MAJOR, (1, 4096, 7, 256) TIME_MAJOR.  Per
shape one Gaussian float32 input of about --mib MiB (n a multiple of Tb, plus the look-ahead), default statistics, no candidates, three
windows each of
  * the geometry's own route and
  * the generic route (set_generic) on the same handle and buffers,
ALTERNATING in the same run (a shape whose own route is the generic one is timed once per window).  Reported: the time per call, the
share of 8 TB/s on 4 S (n + Hs) + 8 S n / Tb bytes, the own / generic time ratio, and -- by arithmetic from the hardware guide's
figures, not from any measurement -- the time the two ceilings would allow: HBM at 8 TB/s on those bytes, and LDS at 256 CUs x 128 B/clk
x 2.4 GHz on the 4-byte LDS accesses of the fused route's first form (one store per staged sample, then one load and one store per
level but the last, which only loads: 2 K - 1 accesses on each of the w / tt staged samples per output).  The two routes' peaks are
compared bit for bit.  No rate is asserted.
usage: python tools/psearch_probe.py [--mib 1024] [--window 0.1]"""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

HBM = 8e12
LDS = 256 * 128 * 2.4e9
SHAPES = [(64, 1024, 10, 1024, 0), (64, 1024, 10, 1024, 1), (16, 512, 13, 4096, 0), (1, 4096, 7, 256, 1)]


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
    ap.add_argument("--mib", type=int, default=1024, help="input MiB per shape")
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clPulseSearch probe: about %d MiB of input per shape, HIP events, windows of >= %.2f s, three windows each, own route / generic "
          "route alternating; ceilings by arithmetic: HBM %.3g B/s, LDS %.3g B/s" % (a.mib, a.window, HBM, LDS))
    for R, D, K, Tb, order in SHAPES:
        S = R * D
        blk = pkg.clPulseSearch(*args, R, D, K, Tb, order)
        Hs = blk.history()
        nb = max(1, (a.mib << 20) // (4 * S * Tb))
        n = nb * Tb
        g = torch.Generator(device="cuda").manual_seed(7)
        d_x = torch.randn((S * (n + Hs),), dtype=torch.float32, device="cuda", generator=g)
        d_y = torch.full((nb * S,), -1, dtype=torch.int64, device="cuda")
        d_z = torch.full_like(d_y, -1)
        route = blk.route()
        fused = route.startswith("tiled")

        def run_own():
            blk.set_generic(False)
            blk.work_device(nb, [d_x], [d_y])

        def run_gen():
            blk.set_generic(True)
            blk.work_device(nb, [d_x], [d_z])

        run_own()
        run_gen()
        torch.cuda.synchronize()
        if not torch.equal(d_y, d_z):
            raise SystemExit("(%d, %d, %d, %d): %s and the generic route differ" % (R, D, K, Tb, route))
        to, tg = [], []
        for _ in range(3):
            if fused:
                to.append(window(run_own, a.window))
            tg.append(window(run_gen, a.window))
        nbytes = 4.0 * S * (n + Hs) + 8.0 * S * nb
        print("(R=%d, D=%d, K=%d, Tb=%d, %s), %d blocks = %d outputs per series, %.3f GB: %s" %
              (R, D, K, Tb, "TIME_MAJOR" if order else "TRIAL_MAJOR", nb, n, nbytes / 1e9, route))
        if fused:
            w, tt = (int(v) for v in re.search(r" w=(\d+) tt=(\d+)", route).groups())
            t_hbm, t_lds = nbytes / HBM, 4.0 * S * n * (w / tt) * (2 * K - 1) / LDS
            print("    own route   %s ms   best %.3f of 8 TB/s; own / generic %.4fx of its time" %
                  (" ".join("%9.3f" % (v * 1e3) for v in to), nbytes / min(to) / HBM, min(to) / min(tg)))
            print("    ceilings    HBM %.3f ms, LDS %.3f ms (%d accesses per output at w / tt = %.2f): %s binds; best = %.2f of it" %
                  (t_hbm * 1e3, t_lds * 1e3, 2 * K - 1, w / tt, "LDS" if t_lds > t_hbm else "HBM", max(t_hbm, t_lds) / min(to)))
        print("    generic     %s ms   best %.4f of 8 TB/s" % (" ".join("%9.3f" % (v * 1e3) for v in tg), nbytes / min(tg) / HBM))
        blk.stop()
        del d_x, d_y, d_z
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
