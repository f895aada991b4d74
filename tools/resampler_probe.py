#!/usr/bin/env python3
"""clRationalResampler probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

For every probe shape (L, M, K), 2^26 outputs per call (input and output together pass the 256 MiB Infinity Cache):
  * GS/s of output and the share of the roofline: the larger of 8 (n_in + n_out) bytes over 8 TB/s and the FMAs over the FP32
    vector peak, over the measured time, labelled with the bound that applies;
  * the same outputs the only way the library could make them before this block: the L-fold zero-stuffed stream through
    mi355_filter_work_dev with decimation M, the faster of use_time 0 and 1, ALTERNATING with the resampler in the same run,
    three windows each.  The stuffed stream of 2^26 outputs is M 2^26 items, so the composition works in pieces of at most
    2^28 stuffed items; its buffer is zeroed once, outside the timing, and a piece costs one strided copy (the zero-stuffing
    kernel, also timed alone) and one filter call;
  * at (1, 1, 65) also clFilter itself; where k_rs_interp serves a shape also k_rs_lds (a handle made with
    MI355_RESAMPLER_GENERAL=1), and at (8, 1, 89) the fallback kernel (MI355_RESAMPLER_PLAIN=1).
Every resampler handle is made with setDebug and its INFO line must name the kernel the row claims.
The last lines assert what the block promises: faster than the composition at every shape with L >= 2.
usage: python tools/resampler_probe.py [--log2n 26] [--window 0.2]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS, PEAK_TFLOPS = 8.0, 157.3
SHAPES = [(8, 1, 89, False, "RRC, 11 symbols at 8 sps"), (8, 1, 89, True, "complex taps"), (2, 1, 65, False, ""),
          (3, 2, 97, False, ""), (160, 147, 3840, False, ""), (147, 160, 3528, False, ""), (1, 1, 65, False, "degenerate")]
STUFF_PIECE = 1 << 28


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


VARIANT_ENV = {"k_rs_plain": "MI355_RESAMPLER_PLAIN", "k_rs_lds": "MI355_RESAMPLER_GENERAL"}


def made(pkg, make, expect, force=False):
    """make() a handle; force: with the tuning variable set that selects `expect` where it is not the default (the library reads
    it when a handle is created).  The handle's INFO line must name `expect`: a probe that times a mislabelled kernel is worse
    than none."""
    lines = []
    for v in VARIANT_ENV.values():
        os.environ.pop(v, None)
    if force:
        os.environ[VARIANT_ENV[expect]] = "1"
    pkg.set_log_callback(lambda level, msg: lines.append(msg))
    try:
        blk = make()
    finally:
        pkg.set_log_callback(None)
        for v in VARIANT_ENV.values():
            os.environ.pop(v, None)
    if not any(m.startswith("clRationalResampler") and expect in m for m in lines):
        raise SystemExit("the kernel '%s' was not selected: %r" % (expect, lines))
    return blk


def taps_of(K, L, cplx):
    k = np.arange(K) - (K - 1) / 2.0
    h = (L * np.sinc(k / L) * np.hamming(K) / L).astype(np.float32)  # a windowed-sinc low-pass at 1 / L, gain L
    return (h * np.exp(0.3j * k)).astype(np.complex64) if cplx else h


class Composition:
    """zero-stuff + clFilter(decimation M) in pieces; pieces hold a multiple of L stuffed items and of M, so every piece starts at
    phase 0 of both"""

    def __init__(self, pkg, args, L, M, h, n_out, d_x, nt):
        import torch
        self.L, self.M, self.K, self.nt, self.d_x, self.n_out = L, M, h.size, nt, d_x, n_out
        cplx = np.iscomplexobj(h)
        self.po = max(L, min(n_out, STUFF_PIECE // M) // L * L)          # outputs per piece: po M / L input items, exactly
        self.pi = self.po * M // L
        items = self.pi + nt - 1 + 1                                      # history-prefixed input of a piece (+1: the window of the last output)
        self.z = torch.zeros((L - 1) + items * L + self.K + M, dtype=torch.complex64, device="cuda")
        self.zv = self.z[L - 1:L - 1 + items * L].view(items, L)[:, 0]   # where the samples go
        self.items = items
        self.start = (L - 1) + (nt - 1) * L - (self.K - 1)               # the filter's history-prefixed input starts here
        self.out = torch.empty(self.po, dtype=torch.complex64, device="cuda")
        self.filters = {}
        for ut in (0, 1):
            try:
                f = (pkg.clComplexFilter(*args, M, h, 1, 0, bool(ut)) if cplx else pkg.clFilter(*args, M, h, 1, 0, bool(ut)))
                self.stuff(0)
                f.work_device(self.po, [self.z[self.start:]], [self.out])
                torch.cuda.synchronize()
                self.filters[ut] = f
            except Exception as e:  # a form the filter does not offer for this shape
                print("    (clFilter use_time=%d not available here: %s)" % (ut, str(e)[:100]))
        self.ut = None

    def stuff(self, piece):
        src = self.d_x[piece * self.pi:piece * self.pi + self.items]
        self.zv[:src.numel()].copy_(src)

    def pieces(self):
        return (self.n_out + self.po - 1) // self.po

    def run(self, ut, stuff=True, filt=True):
        f = self.filters[ut]
        for p in range(self.pieces()):
            n = min(self.po, self.n_out - p * self.po)
            if stuff:
                self.stuff(p)
            if filt:
                f.work_device(n, [self.z[self.start:]], [self.out])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    n_out = 1 << a.log2n
    verdicts = []
    print("clRationalResampler probe: %d outputs per call, HIP events, windows of >= %.2f s, three windows each, alternating" % (n_out, a.window))
    for L, M, K, cplx, note in SHAPES:
        h = taps_of(K, L, cplx)
        nt = -(-K // L)
        kernel = "k_rs_interp" if M == 1 and 4 <= L <= 16 and nt <= 40 else "k_rs_lds"
        blk = made(pkg, lambda: pkg.clRationalResampler(*args, L, M, h, 1), kernel)
        n_in = blk.plan(n_out)[1]
        d_x = torch.complex(torch.randn(n_in + nt + 8, device="cuda"), torch.randn(n_in + nt + 8, device="cuda")).contiguous()
        d_y = torch.empty(n_out, dtype=torch.complex64, device="cuda")

        def rs(b=blk):
            b.set_phase(0)
            b.work_device(n_out, [d_x], [d_y])

        comp = Composition(pkg, args, L, M, h, n_out, d_x, nt)
        # the two paths compute the same thing (first piece, against the resampler's output)
        rs()
        comp.stuff(0)
        ut0 = sorted(comp.filters)[0]
        comp.filters[ut0].work_device(comp.po, [comp.z[comp.start:]], [comp.out])
        torch.cuda.synchronize()
        scale = float(d_y[:comp.po].abs().max())
        diff = float((d_y[:comp.po] - comp.out).abs().max()) / scale
        if not diff < 1e-4:
            raise SystemExit("(%d, %d, %d): resampler and composition disagree, max rel diff %.3g" % (L, M, K, diff))
        for f in comp.filters:  # warm-up of every shape, and which filter form is the faster one
            comp.run(f)
        torch.cuda.synchronize()
        t_ut = {f: window(lambda f=f: comp.run(f), a.window / 4) for f in comp.filters}
        best = min(t_ut, key=t_ut.get)
        rs_t, co_t = [], []
        for _ in range(3):
            rs_t.append(window(rs, a.window))
            co_t.append(window(lambda: comp.run(best), a.window))
        stuff_t = window(lambda: comp.run(best, filt=False), a.window / 4)
        bytes_ = 8.0 * (n_in + n_out)
        flops = n_out * nt * (8.0 if cplx else 4.0)
        t_mem, t_flop = bytes_ / (PEAK_TBS * 1e12), flops / (PEAK_TFLOPS * 1e12)
        t = min(rs_t)
        label = "HBM-bound" if t_mem >= t_flop else "FP32-bound"
        print("(%3d, %3d, %4d) %s%s: %s, %d taps per arm" % (L, M, K, "complex taps" if cplx else "real taps", ", " + note if note and not cplx else "", kernel, nt))
        print("    resampler    %s ms   best %7.1f GS/s of output   %.2f of the %s roofline (%.0f TB/s on %.2f GB%s)" %
              (" ".join("%8.3f" % (v * 1e3) for v in rs_t), n_out / t / 1e9, max(t_mem, t_flop) / t, label, PEAK_TBS, bytes_ / 1e9,
               "" if label == "HBM-bound" else "; bytes alone: %.2f of 8 TB/s" % (t_mem / t)))
        print("    composition  %s ms   zero-stuff + clFilter(use_time=%d, decimation %d) in %d piece(s); use_time: %s; the zero-stuffing copies alone %.3f ms" %
              (" ".join("%8.3f" % (v * 1e3) for v in co_t), best, M, comp.pieces(),
               ", ".join("%d: %.3f ms" % (f, v * 1e3) for f, v in sorted(t_ut.items())), stuff_t * 1e3))
        spread = max(co_t) - min(co_t)
        print("    resampler / composition: %.1fx faster (slowest resampler window %.3f ms, fastest composition window %.3f ms, composition spread %.3f ms)" %
              (min(co_t) / t, max(rs_t) * 1e3, min(co_t) * 1e3, spread * 1e3))
        if L >= 2:
            verdicts.append(((L, M, K, cplx), max(rs_t) + spread < min(co_t)))
        if (L, M, K) == (1, 1, 65):
            for ut in (0, 1):
                f = pkg.clFilter(*args, 1, h, 1, 0, bool(ut))
                tf = min(window(lambda: f.work_device(n_out, [d_x], [d_y]), a.window) for _ in range(3))
                print("    clFilter(use_time=%d) itself: %8.3f ms  %7.1f GS/s   resampler / clFilter time: %.2f" % (ut, tf * 1e3, n_out / tf / 1e9, t / tf))
        for other in ("k_rs_lds", "k_rs_plain"):  # the other kernels on the same shape, same outputs bit for bit
            if other == kernel or (other == "k_rs_plain" and (L, M, K, cplx) != (8, 1, 89, False)):
                continue
            rs()
            want = d_y.clone()
            alt = made(pkg, lambda: pkg.clRationalResampler(*args, L, M, h, 1), other, force=True)
            rs(alt)
            torch.cuda.synchronize()
            same = bool(torch.equal(want.view(torch.int32), d_y.view(torch.int32)))
            tp = [window(lambda: rs(alt), a.window) for _ in range(3)]
            print("    %-11s on the same shape: %s ms   best %7.1f GS/s   (outputs %s those of %s)" %
                  (other, " ".join("%8.3f" % (v * 1e3) for v in tp), n_out / min(tp) / 1e9, "bit-identical to" if same else "DIFFER from", kernel))
        del comp, d_x, d_y
        torch.cuda.empty_cache()
    bad = [s for s, ok in verdicts if not ok]
    print("faster than zero-stuff + clFilter by more than the composition's spread at every shape with L >= 2: %s" % ("yes" if not bad else "NO: %r" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
