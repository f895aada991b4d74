#!/usr/bin/env python3
"""clBeamformer probe, device-resident, HIP events around back-to-back calls after a warm-up of every shape.

Shapes (S, B, F, npol, mode, Ti): (64, 64, 1024, 2, POWER, 1024), (64, 64, 1024, 2, VOLTAGE), (64, 8, 1024, 2, VOLTAGE),
(256, 128, 512, 1, POWER, 256), (16, 16, 64, 1, POWER, 64).  Per shape one int8 input of `--mib` MiB (whole units; VOLTAGE shapes a
quarter of it, their output is up to 4x the input), three windows each, ALTERNATING in the same run:
  * clBeamformer on its own route: the time per call, frames/s, and the share of 8 TB/s on the bytes read (frames + one weight set) plus
    the bytes written;
  * clXEngine on the same frames (mi355_xengine_xcorrelate_n_dev; integration = Ti, 256 for the VOLTAGE shapes), the sibling yardstick,
    with its own share of 8 TB/s on input + matrices.
The first unit of every shape is compared bit for bit with the generic route on the same handle.  No rate is asserted.
usage: python tools/beamform_probe.py [--mib 1024] [--window 0.1]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

PEAK_TBS = 8.0
VOLTAGE, POWER = 0, 1
SHAPES = [(64, 64, 1024, 2, POWER, 1024), (64, 64, 1024, 2, VOLTAGE, 1), (64, 8, 1024, 2, VOLTAGE, 1), (256, 128, 512, 1, POWER, 256),
          (16, 16, 64, 1, POWER, 64)]


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
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    import torch
    pkg = entry.load_package()
    args = (pkg.OCLTYPE_GPU, pkg.OCLDEVICESELECTOR_SPECIFIC, 0, 0)
    print("clBeamformer probe: int8 inputs of up to %d MiB, HIP events, windows of >= %.2f s, three windows each, clBeamformer / clXEngine "
          "alternating" % (a.mib, a.window))
    rng = np.random.default_rng(7)
    for S, B, F, npol, mode, Ti in SHAPES:
        w = rng.integers(-127, 128, size=(F, npol, B, S, 2), dtype=np.int8)
        blk = pkg.clBeamformer(*args, mode, npol, S, F, B, Ti, False, w)
        unit_in = blk.frame_bytes() * Ti
        budget = (a.mib << 20) // (4 if mode == VOLTAGE else 1)
        nunits = max(1, budget // unit_in)
        d_x = torch.randint(-128, 128, (nunits * unit_in,), dtype=torch.int8, device="cuda")
        dt = torch.complex64 if mode == VOLTAGE else torch.float32
        d_y = torch.full((nunits * blk.out_items_per_unit(),), float("nan"), dtype=dt, device="cuda")
        route = blk.route()

        def run_bf():
            blk.work_device(nunits, [d_x], [d_y])

        run_bf()
        torch.cuda.synchronize()
        first = d_y[:blk.out_items_per_unit()].clone()
        assert bool(torch.isfinite(torch.view_as_real(d_y) if mode == VOLTAGE else d_y).all()), "an output was left unwritten"
        blk.set_generic(True)
        chk = torch.empty_like(first)
        blk.work_device(1, [d_x], [chk])
        torch.cuda.synchronize()
        blk.set_generic(False)
        if not torch.equal(first, chk):
            raise SystemExit("(%d, %d, %d, %d): the first unit differs between %s and the generic route" % (S, B, F, npol, route))
        # the sibling: the X-engine on the same frames
        xe, run_xe, xe_bytes, xe_note = None, None, 0.0, ""
        Tx = Ti if mode == POWER else 256
        nint = (nunits * Ti) // Tx
        try:
            xe = pkg.clXEngine(*args, 0, pkg.DTYPE_BYTE, npol, S, 1, 0, F, Tx)
            d_m = torch.empty(nint * xe.get_output_buffer_size(), dtype=torch.complex64, device="cuda")

            def run_xe():
                xe.xcorrelate_n_device(nint, d_x, d_m)

            run_xe()
            torch.cuda.synchronize()
            xe_bytes = float(nint * xe.input_bytes() + d_m.numel() * 8)
        except Exception as e:  # a shape the X-engine does not take is reported, not hidden
            xe_note, run_xe = "clXEngine does not run this shape: %s" % e, None
        tb, tx = [], []
        for _ in range(3):
            tb.append(window(run_bf, a.window))
            if run_xe:
                tx.append(window(run_xe, a.window))
        nbytes = float(nunits * unit_in + w.size + d_y.numel() * d_y.element_size())
        frames = nunits * Ti
        print("(S=%d, B=%d, F=%d, npol=%d, %s%s), %d units = %d frames: %s" %
              (S, B, F, npol, "POWER" if mode == POWER else "VOLTAGE", ", Ti=%d" % Ti if mode == POWER else "", nunits, frames, route))
        print("    clBeamformer  %s ms   best %9.1f kframes/s   %.3f of %.0f TB/s on %.3f GB (read %.3f + written %.3f)" %
              (" ".join("%8.3f" % (v * 1e3) for v in tb), frames / min(tb) / 1e3, nbytes / min(tb) / (PEAK_TBS * 1e12), PEAK_TBS, nbytes / 1e9,
               (nunits * unit_in + w.size) / 1e9, d_y.numel() * d_y.element_size() / 1e9))
        if tx:
            print("    clXEngine     %s ms   best %9.1f kframes/s   %.3f of %.0f TB/s on %.3f GB (integration %d, %d windows); beamformer / X-engine %.3fx of its time" %
                  (" ".join("%8.3f" % (v * 1e3) for v in tx), nint * Tx / min(tx) / 1e3, xe_bytes / min(tx) / (PEAK_TBS * 1e12), PEAK_TBS,
                   xe_bytes / 1e9, Tx, nint, min(tb) / min(tx)))
        else:
            print("    " + xe_note)
        blk.stop()
        if xe is not None:
            xe.stop()
        del d_x, d_y
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
