#!/usr/bin/env python3
"""clSpectralSearch probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (S, N, H, Bb): (1024, 2^20, 5, 1024), (64, 2^22, 5, 4096), (4096, 2^17, 4, 256), (1, 2^20, 5, 1024).  Per shape one unit Gaussian
float32 input of S series of N samples, k_lo = 8, no candidates, three windows each of
  * the whole call (SERIES input, the tiled route, no spectrum output),
  * the harmonic-sum stage alone through SPECTRUM input on the spectrum of the same series, tiled,
  * the same under set_generic,
  * a clFFT handle of N / 2 complex points on the input's bytes (what the block's internal transform does), and
  * a device-to-device copy of the input,
ALTERNATING in the same run.  Reported: the time per leg, the whole call's share of 8 TB/s on 4 S N + 8 S Nb / Bb bytes, and the sum
stage's additions per second on S Nb (2^H - 1) additions per call beside one ceiling taken from the hardware guide's figures and not
from any measurement -- 256 CUs x 128 B/clk of 4-byte LDS reads at 2.4 GHz, one read per addition -- and the ratio of the tiled route's
time to the generic route's.  The two routes' records are compared bit for bit.  No rate is asserted.
usage: python tools/ssearch_probe.py [--window 0.1] [--no-generic] [--shape S,N,H,Bb]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LDS_ADDS = 256 * 128 / 4 * 2.4e9
HBM = 8e12
SHAPES = [(1024, 1 << 20, 5, 1024), (64, 1 << 22, 5, 4096), (4096, 1 << 17, 4, 256), (1, 1 << 20, 5, 1024)]


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
    ap.add_argument("--no-generic", action="store_true", help="leave the generic route out")
    ap.add_argument("--shape", action="append", help="S,N,H,Bb instead of the four shapes; may be given more than once")
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else SHAPES
    print("clSpectralSearch probe: HIP events, windows of >= %.2f s, three windows each, whole / sums tiled / sums generic / clFFT / copy "
          "alternating; ceilings %.3g additions/s (LDS, one 4-byte read per addition), 8 TB/s" % (a.window, LDS_ADDS))
    for S, N, H, Bb in shapes:
        Nb = N // 2
        whole = pkg.clSpectralSearch(*args, S, N, H, Bb, 8, pkg.SSEARCH_SERIES)
        sums = pkg.clSpectralSearch(*args, S, N, H, Bb, 8, pkg.SSEARCH_SPECTRUM)
        fft = pkg.clFFT(Nb, pkg.CLFFT_FORWARD, None, pkg.DTYPE_COMPLEX, *args)
        torch.manual_seed(7)
        d_x = torch.randn(S * N, dtype=torch.float32, device="cuda")
        d_c = torch.empty_like(d_x)
        d_w = torch.empty(S * Nb, dtype=torch.float32, device="cuda")
        d_y, d_t, d_g = (torch.empty(S * whole.records, dtype=torch.int64, device="cuda") for _ in range(3))

        def run_whole():
            whole.work_device([d_x], [d_y])

        def run_tiled():
            sums.set_generic(False)
            sums.work_device([d_w], [d_t])

        def run_gen():
            sums.set_generic(True)
            sums.work_device([d_w], [d_g])

        def run_fft():
            fft.work_device(S, [d_x], [d_c])   # S frames of Nb complex items in, as many out: the bytes of the input

        def run_copy():
            d_c.copy_(d_x)

        whole.work_device([d_x], [d_y, d_w])   # the spectrum the sum legs run on
        run_tiled()
        run_fft()
        run_copy()
        torch.cuda.synchronize()
        if not torch.equal(d_y, d_t):
            raise SystemExit("(%d, %d, %d, %d): the whole call and the sums over its spectrum differ" % (S, N, H, Bb))
        if not a.no_generic:
            run_gen()
            torch.cuda.synchronize()
            if not torch.equal(d_t, d_g):
                raise SystemExit("(%d, %d, %d, %d): the tiled and the generic route differ" % (S, N, H, Bb))
        tw, tt, tg, tf, tc = [], [], [], [], []
        for _ in range(3):
            tw.append(window(run_whole, a.window))
            tt.append(window(run_tiled, a.window))
            if not a.no_generic:
                tg.append(window(run_gen, a.window))
            tf.append(window(run_fft, a.window))
            tc.append(window(run_copy, a.window))
        adds = float(S) * Nb * ((1 << H) - 1)
        nbytes = 4.0 * S * N + 8.0 * S * Nb / Bb
        fm = lambda v: " ".join("%9.3f" % (t * 1e3) for t in v)
        print("(S=%d, N=%d, H=%d, Bb=%d), %.1f MiB of input, scratch %.1f MiB: %s; clFFT %s"
              % (S, N, H, Bb, 4.0 * S * N / 2 ** 20, whole.scratch_bytes / 2 ** 20, whole.route(), whole.fft_route()))
        print("    whole call   %s ms   best %.3f of 8 TB/s on %.1f MiB; %.2fx the copy's time, %.2fx the clFFT leg's"
              % (fm(tw), nbytes / min(tw) / HBM, nbytes / 2 ** 20, min(tw) / min(tc), min(tw) / min(tf)))
        print("    sums tiled   %s ms   best %.3g additions/s = %.3f of the LDS ceiling; %.2fx the clFFT leg's time"
              % (fm(tt), adds / min(tt), adds / min(tt) / LDS_ADDS, min(tt) / min(tf)))
        if tg:
            print("    sums generic %s ms   best %.3g additions/s; tiled / generic %.3fx of its time%s"
                  % (fm(tg), adds / min(tg), min(tt) / min(tg), "" if min(tt) <= min(tg) else "  ** the tiled route LOSES here **"))
        else:
            print("    sums generic not measured")
        print("    clFFT        %s ms   %d frames of %d complex points" % (fm(tf), S, Nb))
        print("    copy         %s ms   of the %.1f MiB input" % (fm(tc), 4.0 * S * N / 2 ** 20))
        for b in (whole, sums, fft):
            b.stop()
        del d_x, d_c, d_w, d_y, d_t, d_g
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
