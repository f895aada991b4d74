#!/usr/bin/env python3
"""Per-workgroup stamps of the persistent clFFT schedule (tuning aid, needs a GPU).

Runs the headline shape (forward 4096 points, Blackman window, shift, 16384 frames) with MI355_FFT_TS=1 for each schedule
(MI355_FFT_SCHED=0: static grid stride, 1: dynamic claims), the schedules interleaved round by round after warming the clocks
(a stamped launch is synchronous, so its clocks sit below the back-to-back rate), and prints for each:
  - the spread of the workgroup end times (median, 95th percentile, max; us after the first start);
  - the time per frame group per CU (the two workgroups of a CU, found by their hardware ids), by XCD.

usage: python tools/fft_stamps.py [--frames 16384] [--n 4096] [--rounds 5] [--sched 0,1]
"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import __graft_entry__ as e  # noqa: E402

TICK_US = 0.01  # the stamps count a 100 MHz wall clock


def parse(path):
    """-> list of launches, each (header dict, array of rows [block, hw, start, end, groups], list of per-8-group stamps)"""
    launches = []
    for line in open(path):
        if line.startswith("#"):
            f = line.split()[1:]
            launches.append((dict(zip(f[0::2], map(int, f[1::2]))), [], []))
        else:
            v = [int(x) for x in line.split()]
            launches[-1][1].append(v[:5])
            launches[-1][2].append(v[5:])
    return [(h, np.array(r, dtype=np.int64), s) for h, r, s in launches]


def report(h, rows, marks):
    t0 = rows[:, 2].min()
    end = (rows[:, 3] - t0) * TICK_US
    start = (rows[:, 2] - t0) * TICK_US
    groups = rows[:, 4]
    print("  sched %d: %d workgroups, %d groups, groups per workgroup min / median / max %d / %d / %d" % (
        h["sched"], len(rows), h["ngroups"], groups.min(), int(np.median(groups)), groups.max()))
    print("    start  (us after first start): median %6.2f  p95 %6.2f  max %6.2f" % (
        np.median(start), np.percentile(start, 95), start.max()))
    print("    end    (us after first start): min %7.2f  median %7.2f  p95 %7.2f  max %7.2f  spread max - median %5.2f  max - min %5.2f" % (
        end.min(), np.median(end), np.percentile(end, 95), end.max(), end.max() - np.median(end), end.max() - end.min()))
    # per CU: the workgroups that share (XCC, SE, CU); time per group = the CU's span (first start to last end) / groups it did
    cu = {}
    for r in rows:
        cu.setdefault(int(r[1]), []).append(r)
    by_xcd = {}
    for key, rs in cu.items():
        rs = np.array(rs)
        us_per_group = float((rs[:, 3].max() - rs[:, 2].min()) * TICK_US / max(rs[:, 4].sum(), 1))
        by_xcd.setdefault(key >> 16, []).append(us_per_group)
    allr = np.concatenate([np.array(v) for v in by_xcd.values()])
    print("    %d CUs (%s workgroups per CU); CU time per group, us: median %.3f, min %.3f, max %.3f (max/min %.3f)" % (
        len(cu), "/".join(sorted({str(len(v)) for v in cu.values()})), np.median(allr), allr.min(), allr.max(), allr.max() / allr.min()))
    for x in sorted(by_xcd):
        v = np.array(by_xcd[x])
        print("      XCD %d: %2d CUs  median %.3f  min %.3f  max %.3f" % (x, len(v), np.median(v), v.min(), v.max()))
    # XCD by block index under the round-robin dispatch, for comparison with the hardware ids
    bx = rows[:, 0] % 8
    print("    end by blockIdx % 8 (median us): " + " ".join("%d:%.2f" % (x, np.median(end[bx == x])) for x in range(8)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sched", default="0,1")
    a = ap.parse_args()
    pkg = e.load_package()
    n = a.n
    w = np.blackman(n).astype(np.float32)
    blk = pkg.clFFT(n, pkg.CLFFT_FORWARD, w, pkg.DTYPE_COMPLEX, 1, 2, 0, 0, 0, 1, True)
    x = torch.randn(a.frames * n, 2, device="cuda")
    y = torch.empty_like(x)
    for _ in range(200):  # warm clocks
        blk.work_device(a.frames, [x], [y])
    torch.cuda.synchronize()
    print("clFFT %d forward, window + shift, %d frames per launch; the schedules interleaved: per round and schedule 10 launches"
          " without stamps, then one stamped (synchronous) launch; the last round is shown in full" % (n, a.frames))
    scheds = a.sched.split(",")
    paths = {}
    for sched in scheds:
        fd, paths[sched] = tempfile.mkstemp(suffix=".txt")
        os.close(fd)
    for _ in range(a.rounds):
        for sched in scheds:
            os.environ["MI355_FFT_SCHED"] = sched
            for _ in range(10):  # the schedule's own clocks, no stamps
                blk.work_device(a.frames, [x], [y])
            os.environ.update({"MI355_FFT_TS": "1", "MI355_FFT_TS_FILE": paths[sched]})
            blk.work_device(a.frames, [x], [y])
            for k in ("MI355_FFT_TS", "MI355_FFT_TS_FILE", "MI355_FFT_SCHED"):
                os.environ.pop(k, None)
    for sched in scheds:
        launches = parse(paths[sched])
        os.unlink(paths[sched])
        if not launches:
            print("  sched %s: no stamps (not the persistent schedule?)" % sched)
            continue
        report(*launches[-1])
        spreads = [((r[:, 3].max() - np.median(r[:, 3])) * TICK_US) for _, r, _ in launches]
        lens = [((r[:, 3].max() - r[:, 2].min()) * TICK_US) for _, r, _ in launches]
        print("    all %d rounds: first start to last end %s us; end spread max - median %s us" % (
            len(launches), " ".join("%.1f" % v for v in lens), " ".join("%.2f" % v for v in spreads)))

if __name__ == "__main__":
    main()
