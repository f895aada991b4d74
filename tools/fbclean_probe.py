#!/usr/bin/env python3
"""clFilterbankCleaner probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (R, F, Tb): (64, 1024, 256), (16, 4096, 256), (64, 1024, 64), (1, 1024, 1024).  Per shape one gamma-distributed float32
filterbank of about --mib MiB (n a multiple of Tb), limits 1 +- 4 (2 / sqrt(Tb)) with nd = 16, td = 5, zero-DM on, all three optional
outputs, out of place, three windows each of
  * the slab route,
  * the generic route (set_generic) on the same handle and buffers, and
  * a device-to-device copy of the input to the output: the same 8 bytes per sample,
ALTERNATING in the same run.  Reported: the time per call, the share of 8 TB/s on 8 bytes per sample (one read, one write: the floor if
phase B's second read of a slab comes from the caches; 12 bytes per sample if it comes from HBM), and the ratio to the copy.  The two
routes' outputs are compared bit for bit.  No rate is asserted.  --pmc-shape I runs shape I's slab route only, a few calls and nothing
else: for a counter run of its own (rocprofv3 --pmc FETCH_SIZE).
usage: python tools/fbclean_probe.py [--mib 1024] [--window 0.1] [--pmc-shape I]"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

HBM = 8e12
SHAPES = [(64, 1024, 256), (16, 4096, 256), (64, 1024, 64), (1, 1024, 1024)]


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
    ap.add_argument("--pmc-shape", type=int, default=-1, help="run this shape's slab route only, 3 calls")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clFilterbankCleaner probe: about %d MiB of input per shape, HIP events, windows of >= %.2f s, three windows each, slab / generic / "
          "copy alternating; shares are of %.3g B/s on 8 bytes per sample" % (a.mib, a.window, HBM))
    shapes = SHAPES if a.pmc_shape < 0 else [SHAPES[a.pmc_shape]]
    for R, F, Tb in shapes:
        w = 4.0 * 2.0 / math.sqrt(Tb)
        blk = pkg.clFilterbankCleaner(*args, R, F, Tb, 16.0, 1.0 - w, 1.0 + w, 5.0, 1)
        nb = max(1, (a.mib << 20) // (4 * R * F * Tb))
        n = nb * Tb
        torch.manual_seed(7)
        d_x = torch.distributions.Gamma(torch.tensor(16.0, device="cuda"), torch.tensor(16.0, device="cuda")).sample((n * R * F,)).to(torch.float32)
        d_y, d_z = torch.empty_like(d_x), torch.empty_like(d_x)
        outs = [[torch.empty(nb * R * F, dtype=torch.int8, device="cuda"), torch.empty(n * R, dtype=torch.int8, device="cuda"),
                 torch.empty(2 * nb * R * F, dtype=torch.float32, device="cuda")] for _ in range(2)]
        route = blk.route()

        def run_slab():
            blk.set_generic(False)
            blk.work_device(n, [d_x], [d_y] + outs[0])

        def run_gen():
            blk.set_generic(True)
            blk.work_device(n, [d_x], [d_z] + outs[1])

        def run_copy():
            d_z.copy_(d_x)

        if a.pmc_shape >= 0:
            for _ in range(3):
                run_slab()
            torch.cuda.synchronize()
            print("(R=%d, F=%d, Tb=%d): 3 calls of %s, %d slabs of %d bytes each, %.0f input bytes per call" % (R, F, Tb, route, nb * R, 4 * Tb * F, 4.0 * n * R * F))
            return 0
        run_slab()
        run_gen()
        torch.cuda.synchronize()
        same = torch.equal(d_y.view(torch.int32), d_z.view(torch.int32)) and all(torch.equal(p.view(torch.int8), q.view(torch.int8)) for p, q in zip(*outs))
        if not same:
            raise SystemExit("(%d, %d, %d): %s and the generic route differ" % (R, F, Tb, route))
        run_copy()
        ts, tg, tc = [], [], []
        for _ in range(3):
            ts.append(window(run_slab, a.window))
            tg.append(window(run_gen, a.window))
            tc.append(window(run_copy, a.window))
        nbytes = 8.0 * n * R * F
        fm = lambda v: " ".join("%9.3f" % (t * 1e3) for t in v)
        print("(R=%d, F=%d, Tb=%d), %d blocks = %d samples, %d slabs, %.3f GB read + written: %s" % (R, F, Tb, nb, n, nb * R, nbytes / 1e9, route))
        print("    slab        %s ms   best %.3f of 8 TB/s; %.2fx the copy's time" % (fm(ts), nbytes / min(ts) / HBM, min(ts) / min(tc)))
        print("    generic     %s ms   best %.4f of 8 TB/s; slab / generic %.4fx of its time" % (fm(tg), nbytes / min(tg) / HBM, min(ts) / min(tg)))
        print("    copy        %s ms   best %.3f of 8 TB/s" % (fm(tc), nbytes / min(tc) / HBM))
        blk.stop()
        del d_x, d_y, d_z, outs
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
