#!/usr/bin/env python3
"""clXCorrelate probe: (1) per-call time of the host path at the GRC defaults (8192 items, max search 512 = 1024 lags, complex,
2 inputs, decim 1), (2) TFLOP/s of mi355_xcorr_td_work_dev on the large shape (2^20 items, max search 4096, 4 complex inputs,
8 frames per call), counting only the overlapping products (2 FLOP each).
usage: python tools/xcorr_td_probe.py [--iters N]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TF = 157.3  # fp32 matrix / vector peak of the MI355X


def overlap_macs(n, m):
    return sum(n - abs(s) for s in range(-m, m) if abs(s) < n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0, False)
    rng = np.random.default_rng(0)

    n = 8192
    blk = pkg.clXCorrelate(*args, 2, n, pkg.DTYPE_COMPLEX, 8, 512, 1, False)
    ins = [(rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) for _ in range(2)]
    for _ in range(20):
        blk.work(n, ins)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        blk.work(n, ins)
    dt = (time.perf_counter() - t0) / a.iters
    print("host path, GRC defaults (N=8192, 1024 lags, complex, 2 inputs): %.1f us per work() call" % (dt * 1e6))
    blk.stop()

    n, k, nf = 1 << 20, 4, 8
    blk = pkg.clXCorrelate(*args, k, n, pkg.DTYPE_COMPLEX, 8, 4096, 1, False)
    m = blk.max_shift
    d_in = [torch.complex(torch.randn(nf * n, device="cuda"), torch.randn(nf * n, device="cuda")).contiguous() for _ in range(k)]
    corr = torch.empty(nf * (k - 1), dtype=torch.float32, device="cuda")
    lags = torch.empty(nf * (k - 1), dtype=torch.int32, device="cuda")
    for _ in range(3):
        blk.work_device(nf, d_in, corr, lags)
    torch.cuda.synchronize()
    reps = 10
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        blk.work_device(nf, d_in, corr, lags)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1e3 / reps
    macs = overlap_macs(n, m) * (k - 1) * nf
    tf = 2 * macs / sec / 1e12
    print("work_dev, N=2^20, %d lags, 4 complex inputs, 8 frames: %.3f ms per call, %.3g overlapping MACs, %.1f TFLOP/s = %.2f of the "
          "%.1f TF fp32 peak" % (2 * m, sec * 1e3, macs, tf, tf / PEAK_TF, PEAK_TF))


if __name__ == "__main__":
    main()
