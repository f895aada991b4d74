#!/usr/bin/env python3
"""clAccelResampler probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (S, N, A per call): (1024, 2^20, 1), (64, 2^20, 16), (64, 2^22, 8), (4096, 2^17, 4), (1, 2^20, 64).  Per shape one input of S
series of N random 32-bit words and the ladder of A trials that mi355_accel_trials gives at tol = 1 sample (tsamp 64 us, centred on
zero acceleration), three windows each of
  * the tiled route,
  * the generic route, and
  * a device-to-device copy of the same output bytes (4 S N A),
ALTERNATING in the same run.  Reported: the time per leg, the share of 8 TB/s on 4 S N (A + 1) bytes (the input read once, every output
written once), and the ratios tiled / generic and tiled / copy.  The two routes' outputs are compared bit for bit.  With --chain the
shape (64, 2^20, 16) is followed by clSpectralSearch (H = 5, Bb = 1024, k_lo = 8) on its 1024 output rows: the resampler's share of the
pair's time.  No rate is asserted.
usage: python tools/accel_probe.py [--window 0.1] [--no-generic] [--chain] [--shape S,N,A]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

HBM = 8e12
TSAMP = 64e-6
SHAPES = [(1024, 1 << 20, 1), (64, 1 << 20, 16), (64, 1 << 22, 8), (4096, 1 << 17, 4), (1, 1 << 20, 64)]
CHAIN = (64, 1 << 20, 16)


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


def ladder(pkg, N, A):
    """A trials, one sample apart at mid-observation, j = -(A // 2) .. A - A // 2 - 1"""
    da = 8 * pkg.ACCEL_LIGHT_M_S / (TSAMP * N * N)
    c, count = pkg.accel_trials(N, TSAMP, (-(A // 2) - 0.25) * da, (A - A // 2 - 1 + 0.25) * da, 1.0)
    if count != A or 0 not in c.tolist():
        raise SystemExit("the ladder holds %d trials, %d were asked for" % (count, A))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--no-generic", action="store_true", help="leave the generic route out")
    ap.add_argument("--chain", action="store_true", help="clSpectralSearch behind the resampler at (64, 2^20, 16)")
    ap.add_argument("--shape", action="append", help="S,N,A instead of the five shapes; may be given more than once")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else SHAPES
    print("clAccelResampler probe: HIP events, windows of >= %.2f s, three windows each, tiled / generic / copy alternating; 8 TB/s" % a.window)
    fm = lambda v: " ".join("%9.3f" % (t * 1e3) for t in v)
    for S, N, A in shapes:
        blk = pkg.clAccelResampler(*args, S, N, ladder(pkg, N, A))
        torch.manual_seed(7)
        d_x = torch.randint(-2 ** 31, 2 ** 31 - 1, (S * N,), dtype=torch.int32, device="cuda")
        d_t, d_g = (torch.empty(S * A * N, dtype=torch.int32, device="cuda") for _ in range(2))
        route = {}

        def run_tiled():
            blk.set_generic(False)
            blk.work_device([d_x], [d_t])

        def run_gen():
            blk.set_generic(True)
            blk.work_device([d_x], [d_g])

        def run_copy():
            d_g.copy_(d_t)

        run_tiled()
        route["tiled"] = blk.route()
        if not a.no_generic:
            run_gen()
            torch.cuda.synchronize()
            if not torch.equal(d_t, d_g):
                raise SystemExit("(%d, %d, %d): the tiled and the generic route differ" % (S, N, A))
        run_copy()
        torch.cuda.synchronize()
        tt, tg, tc = [], [], []
        for _ in range(3):
            tt.append(window(run_tiled, a.window))
            if not a.no_generic:
                tg.append(window(run_gen, a.window))
            tc.append(window(run_copy, a.window))
        nbytes = 4.0 * S * N * (A + 1)
        print("(S=%d, N=%d, A=%d), %.1f MiB in, %.1f MiB out: %s" % (S, N, A, 4.0 * S * N / 2 ** 20, 4.0 * S * N * A / 2 ** 20, route["tiled"]))
        print("    tiled    %s ms   best %.3f of 8 TB/s on %.1f MiB; %.2fx the copy's time" % (fm(tt), nbytes / min(tt) / HBM, nbytes / 2 ** 20,
                                                                                                min(tt) / min(tc)))
        if tg:
            print("    generic  %s ms   best %.3f of 8 TB/s; tiled / generic %.3fx of its time%s"
                  % (fm(tg), nbytes / min(tg) / HBM, min(tt) / min(tg), "" if min(tt) <= min(tg) else "  ** the tiled route LOSES here **"))
        else:
            print("    generic  not measured")
        print("    copy     %s ms   of the %.1f MiB output (read and written: %.3f of 8 TB/s on twice its bytes)"
              % (fm(tc), 4.0 * S * N * A / 2 ** 20, 8.0 * S * N * A / min(tc) / HBM))
        if a.chain and (S, N, A) == CHAIN:
            ss = pkg.clSpectralSearch(*args, S * A, N, 5, 1024, 8, pkg.SSEARCH_SERIES)
            d_f = torch.randn(S * N, dtype=torch.float32, device="cuda")
            d_r = d_t.view(torch.float32)
            d_y = torch.empty(S * A * ss.records, dtype=torch.int64, device="cuda")
            blk.set_generic(False)

            def run_res():
                blk.work_device([d_f], [d_r])

            def run_search():
                ss.work_device([d_r], [d_y])

            def run_pair():
                run_res()
                run_search()

            run_pair()
            torch.cuda.synchronize()
            tr, ts, tp = [], [], []
            for _ in range(3):
                tr.append(window(run_res, a.window))
                ts.append(window(run_search, a.window))
                tp.append(window(run_pair, a.window))
            print("    chain    resampler %s ms, clSpectralSearch on the %d rows %s ms, the pair %s ms: the resampler is %.3f of the search's "
                  "time, %.3f of the pair's" % (fm(tr), S * A, fm(ts), fm(tp), min(tr) / min(ts), min(tr) / min(tp)))
            ss.stop()
            del d_f, d_y
        blk.stop()
        del d_x, d_t, d_g
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
