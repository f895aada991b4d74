#!/usr/bin/env python3
"""clPeriodSearch probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (S, p_lo..p_hi, L, K): (64, 250..251, 12, 7), (1024, 64..79, 10, 5), (16, 4000..4003, 8, 8), (1, 256..511, 11, 6).  Per shape
one gamma-distributed float32 input of S series of 2^L p_hi samples, no profiles, three windows each of
  * the fused route,
  * the generic route (set_generic) on the same handle and buffers, and
  * a device-to-device copy of the input to a buffer of its size,
ALTERNATING in the same run.  Reported: the time per call, the additions per second on S sum_p 2^L p (L + K - 1) additions per call
beside one ceiling taken from the hardware guide's figures and not from any measurement -- 256 CUs x 128 B/clk of 4-byte LDS reads at
2.4 GHz, one read per addition (the fused route reads three values per two additions in its stages and one per addition in its
boxcars) -- the ratio of the fused route's time to the generic route's and to the copy's.  The two routes' records are compared bit
for bit.  No rate is asserted.
usage: python tools/ffa_probe.py [--window 0.1] [--no-generic] [--shape S,p_lo,p_hi,L,K]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LDS_ADDS = 256 * 128 / 4 * 2.4e9
SHAPES = [(64, 250, 251, 12, 7), (1024, 64, 79, 10, 5), (16, 4000, 4003, 8, 8), (1, 256, 511, 11, 6)]


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
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--no-generic", action="store_true", help="leave the generic route out (it takes most of the run)")
    ap.add_argument("--shape", action="append", help="S,p_lo,p_hi,L,K instead of the four shapes; may be given more than once")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else SHAPES
    print("clPeriodSearch probe: HIP events, windows of >= %.2f s, three windows each, fused / generic / copy alternating; ceiling %.3g "
          "additions/s (LDS, one 4-byte read per addition)" % (a.window, LDS_ADDS))
    for S, p_lo, p_hi, L, K in shapes:
        blk = pkg.clPeriodSearch(*args, S, p_lo, p_hi, L, K)
        torch.manual_seed(7)
        d_x = torch.empty(S * blk.N, dtype=torch.float32, device="cuda").exponential_(0.25)
        d_c = torch.empty_like(d_x)
        d_y, d_z = (torch.empty(S * blk.records, dtype=torch.int64, device="cuda") for _ in range(2))
        route = blk.route()

        def run_fused():
            blk.set_generic(False)
            blk.work_device([d_x], [d_y])

        def run_gen():
            blk.set_generic(True)
            blk.work_device([d_x], [d_z])

        def run_copy():
            d_c.copy_(d_x)

        run_fused()
        run_copy()
        torch.cuda.synchronize()
        if not a.no_generic:
            run_gen()
            torch.cuda.synchronize()
            if not torch.equal(d_y, d_z):
                raise SystemExit("(%d, %d..%d, %d, %d): %s and the generic route differ" % (S, p_lo, p_hi, L, K, route))
        tf, tg, tc = [], [], []
        for _ in range(3):
            tf.append(window(run_fused, a.window))
            if not a.no_generic:
                tg.append(window(run_gen, a.window, cap=2))
            tc.append(window(run_copy, a.window))
        adds = float(S) * sum((p << L) * (L + K - 1) for p in range(p_lo, p_hi + 1))
        fm = lambda v: " ".join("%9.3f" % (t * 1e3) for t in v)
        print("(S=%d, p=%d..%d, L=%d, K=%d), %.1f MiB of input, %.3g additions per call, scratch %.1f MiB: %s"
              % (S, p_lo, p_hi, L, K, 4.0 * S * blk.N / 2 ** 20, adds, blk.scratch_bytes / 2 ** 20, route))
        print("    fused       %s ms   best %.3g additions/s = %.3f of the LDS ceiling; %.2fx the copy's time"
              % (fm(tf), adds / min(tf), adds / min(tf) / LDS_ADDS, min(tf) / min(tc)))
        if tg:
            print("    generic     %s ms   best %.3g additions/s; fused / generic %.4fx of its time%s"
                  % (fm(tg), adds / min(tg), min(tf) / min(tg), "" if min(tf) <= min(tg) else "  ** the fused route LOSES here **"))
        else:
            print("    generic     not measured")
        print("    copy        %s ms   of the %.1f MiB input" % (fm(tc), 4.0 * S * blk.N / 2 ** 20))
        blk.stop()
        del d_x, d_c, d_y, d_z
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
