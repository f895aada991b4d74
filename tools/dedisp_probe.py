#!/usr/bin/env python3
"""clDedisperser probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (R, F, D): (64, 1024, 1024), (16, 4096, 512), (1, 256, 4096) on an L-band filterbank, 1200 - 1500 MHz at 1 ms, the delay table
and max_delay from the library's own helper (dispersion measures 0 .. about 1023 pc cm^-3 in equal steps).  Per shape one Gaussian
float32 input of n + max_delay samples and a TIME_MAJOR output, three windows each of
  * the table's own route (tiled for these tables) and
  * the generic route (set_generic) on the same handle and buffers,
ALTERNATING in the same run.  Reported: the time per call, additions per second (n R D F per call; -1 entries: none here), the share of
two ceilings taken from the hardware guide's figures and not from any measurement -- 256 CUs x 128 B/clk of 4-byte LDS reads at 2.4 GHz
= 1.97e13 one-read additions per second, and four times that for the vector ALUs -- and the tiled / generic time ratio.  The two
routes' outputs are compared bit for bit.  No rate is asserted.
usage: python tools/dedisp_probe.py [--n 1024] [--window 0.1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LDS_ADDS = 256 * 128 / 4 * 2.4e9
VALU_ADDS = 4 * LDS_ADDS
SHAPES = [(64, 1024, 1024), (16, 4096, 512), (1, 256, 4096)]
F0_MHZ, BW_MHZ, TSAMP, TOP_DM = 1200.0, 300.0, 1e-3, 1023.0


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
    ap.add_argument("--n", type=int, default=1024, help="outputs per call")
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clDedisperser probe: %d outputs per call, HIP events, windows of >= %.2f s, three windows each, own route / generic route "
          "alternating; ceilings %.3g (LDS, one 4-byte read per addition) and %.3g (vector ALU) additions/s" % (a.n, a.window, LDS_ADDS, VALU_ADDS))
    for R, F, D in SHAPES:
        tab, H = pkg.dedisp_delays(F0_MHZ, BW_MHZ / F, F, TSAMP, np.linspace(0.0, TOP_DM, D))
        blk = pkg.clDedisperser(*args, R, F, D, H, pkg.DEDISP_TIME_MAJOR, tab)
        n = a.n
        g = torch.Generator(device="cuda").manual_seed(7)
        d_x = torch.randn(((n + H) * R * F,), dtype=torch.float32, device="cuda", generator=g)
        d_y = torch.full((n * R * D,), float("nan"), dtype=torch.float32, device="cuda")
        d_z = torch.full_like(d_y, float("nan"))
        route = blk.route()

        def run_own():
            blk.set_generic(False)
            blk.work_device(n, [d_x], [d_y])

        def run_gen():
            blk.set_generic(True)
            blk.work_device(n, [d_x], [d_z])

        run_own()
        run_gen()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(d_y).all()), "an output was left unwritten"
        if not torch.equal(d_y, d_z):
            raise SystemExit("(%d, %d, %d): %s and the generic route differ" % (R, F, D, route))
        to, tg = [], []
        for _ in range(3):
            to.append(window(run_own, a.window))
            tg.append(window(run_gen, a.window))
        adds = float(n) * R * D * F
        print("(R=%d, F=%d, D=%d), max_delay %d, %d outputs = %.3g additions, input %.3f GB, output %.3f GB: %s" %
              (R, F, D, H, n, adds, d_x.numel() * 4 / 1e9, d_y.numel() * 4 / 1e9, route))
        print("    own route   %s ms   best %.3g additions/s = %.3f of the LDS ceiling, %.3f of the vector-ALU ceiling" %
              (" ".join("%9.3f" % (v * 1e3) for v in to), adds / min(to), adds / min(to) / LDS_ADDS, adds / min(to) / VALU_ADDS))
        print("    generic     %s ms   best %.3g additions/s = %.3f of the LDS ceiling; own / generic %.3fx of its time" %
              (" ".join("%9.3f" % (v * 1e3) for v in tg), adds / min(tg), adds / min(tg) / LDS_ADDS, min(to) / min(tg)))
        blk.stop()
        del d_x, d_y, d_z
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
