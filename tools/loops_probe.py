#!/usr/bin/env python3
"""clSignalSource / clCostasLoop probe, device-resident, HIP-event timing after warm-up calls of every shape:
(1) signal source, complex, 2^26 items: GS/s and the share of 8 TB/s at 8 B/item, the rotation kernel against the literal
    one-sincos-per-item form (a handle created with MI355_SIGSOURCE_LITERAL=1), alternating;
(2) Costas, one stream, 8192 and 2^20 items: MS/s of k_costas_one against the one-lane form (a handle created with
    MI355_COSTAS_ONE_LANE=1);
every variant handle is created with setDebug and its INFO line must name the kernel it was meant to select;
(3) Costas, 64 / 1024 / 4096 streams of 65536 items: aggregate MS/s.
usage: python tools/loops_probe.py [--reps N]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS = 8.0  # HBM3E peak of the MI355X


def timed(fn, reps, warm=3):
    """seconds per call: events around `reps` back-to-back calls, the best of three windows"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 1e3 / reps)
    return best


def created_with(pkg, name, on, make, expect):
    """make() with the tuning variable `name` set (or unset): the library reads it once, when a handle is created.  The block is
    made with setDebug, and the INFO line of its create must name the variant `expect` -- a probe that times a mislabelled
    kernel is worse than none."""
    lines = []
    os.environ.pop(name, None)
    if on:
        os.environ[name] = "1"
    pkg.set_log_callback(lambda level, msg: lines.append(msg))
    try:
        blk = make()
    finally:
        pkg.set_log_callback(None)
        os.environ.pop(name, None)
    if not any(expect in m for m in lines):
        raise SystemExit("the variant '%s' was not selected: %r" % (expect, lines))
    return blk


def same_bits(a, b):
    import torch
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)

    n = 1 << 26
    variants = [("rotation (1 sincos per 16 items)", False), ("literal (1 sincos per item)", True)]
    srcs = [created_with(pkg, "MI355_SIGSOURCE_LITERAL", lit, lambda: pkg.clSignalSource(pkg.DTYPE_COMPLEX, *args, 48000.0, 1, 1234.5, 1.0, 1),
                         "literal" if lit else "rotation") for _, lit in variants]
    out = torch.empty(n, dtype=torch.complex64, device="cuda")
    # did the variable take effect?  Items off a thread's base item differ in the last float bit here and there between the forms.
    probe = [torch.empty(1 << 20, dtype=torch.complex64, device="cuda") for _ in srcs]
    for src, buf in zip(srcs, probe):
        src.work_device(1 << 20, [], [buf])
        src.set_phase(0.0)
    torch.cuda.synchronize()
    if same_bits(*probe):
        print("WARNING: rotation and literal outputs are bit-identical over 2^20 items: the variants were probably not selected")
    else:
        diff = float((probe[0] - probe[1]).abs().max())
        print("variants differ as they should: max |rotation - literal| over 2^20 items = %.3g" % diff)
    for rnd in range(2):  # alternating: rotation, literal, rotation, literal
        for (name, _), src in zip(variants, srcs):
            sec = timed(lambda: src.work_device(n, [], [out]), a.reps)
            print("clSignalSource complex, 2^26 items, %-34s %8.3f ms  %7.1f GS/s  %.2f of %.0f TB/s" %
                  (name + ":", sec * 1e3, n / sec / 1e9, n * 8 / sec / 1e12 / PEAK_TBS, PEAK_TBS))
    del out, probe

    variants = [("k_costas_one (wave, tiles ahead)", False), ("one lane of k_costas_lanes", True)]
    for n in (8192, 1 << 20):
        x = torch.complex(torch.randn(n, device="cuda"), torch.randn(n, device="cuda")).contiguous()
        y = torch.empty_like(x)
        loops = [created_with(pkg, "MI355_COSTAS_ONE_LANE", lane, lambda: pkg.clCostasLoop(*args, 0.0628, 4, 1),
                              "k_costas_lanes" if lane else "k_costas_one") for _, lane in variants]
        for rnd in range(2):
            for (name, _), loop in zip(variants, loops):
                sec = timed(lambda: loop.work_device(n, [x], [y]), max(2, a.reps // 4))
                print("clCostasLoop order 4, 1 stream, %7d items, %-34s %9.1f us  %6.2f MS/s   (reference, one OpenCL work-item: 0.7 MS/s)" %
                      (n, name + ":", sec * 1e6, n / sec / 1e6))

    n = 65536
    for streams in (64, 1024, 4096):
        x = torch.complex(torch.randn(n * streams, device="cuda"), torch.randn(n * streams, device="cuda")).contiguous()
        y = torch.empty_like(x)
        for order in (2, 4):
            loop = pkg.clCostasLoop(*args, 0.0628, order, 0, streams)
            sec = timed(lambda: loop.work_device(n, [x], [y]), max(2, a.reps // 10), warm=1)
            print("clCostasLoop order %d, %4d streams x %d items: %8.2f ms  %8.1f MS/s aggregate  %6.2f MS/s per stream" %
                  (order, streams, n, sec * 1e3, n * streams / sec / 1e6, n / sec / 1e6))


if __name__ == "__main__":
    main()
