"""The cases that run the switch-selected kernels and the multi-piece calls against float64 (tests/switches.py is the inventory).

One function per case: it takes the package and the oracle, builds the block on a DEBUG context (so the library's INFO lines reach the log
callback), runs it on NaN-filled outputs and returns

    {"taken": True / False / None, "evidence": text, "checks": [[label, error, bound], ...]}

taken    whether the library itself said that the switch was acted on: route(), last_route(), the INFO line of create, or the line
         "switch NAME: ..." a launch-time switch emits the first time a non-default value is used.  None: the library has nothing to say
         (grid sizes, schedules with identical results) -- for those the inventory test is what catches a misspelt name.
checks   every error with the bound it must meet: conftest.relerr against float64 (the oracle with f64=True, numpy's float64 FFT and a float64
         convolution where the oracle has no such mode or cannot run the size), or 0.0 / 1.0 with bound 0.0 for a bit-for-bit comparison.

The same functions are called in two ways.  tests/test_switches_gpu.py calls the cases of INPROC under monkeypatch.setenv (switches read
at create or per call, whose evidence does not depend on a once-per-process line).  tests/test_switches_once_gpu.py starts one child
process per group of CHILD (`python tests/switch_cases.py GROUP`): the group's environment holds the switches that are read once per
process, a case's own environment (read at create or per call) is set through os.environ inside the child; the child prints one JSON line
per case.  Tolerances: DESIGN.md, "Tolerances" -- 1e-5 for every float path; 2e-6 / 3e-6 for power-of-two / mixed-radix transforms, which is
what the default routes of the same lengths meet in tests/test_fft_gpu.py; bit-exact for int8 and for whatever is promised identical.
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

GPU_ARGS = (1, 2, 0, 0)
TOL = 1e-5
LOG = []        # every line the library logged since install_log()
INPROC = {}     # name -> Case
CHILD = {}      # name -> Case
GROUPS = {}     # child group -> environment of its process
FAULT_EXIT = 70  # exit status of a child that stopped at a HIP error


class Case:
    def __init__(self, name, fn, env, switches, group, taken):
        self.name, self.fn, self.env, self.switches, self.group, self.taken = name, fn, env, switches, group, taken


def add(name, fn, env=None, group=None, switches=None, taken=True):
    """register a case.  env: what the case itself sets (create / call switches); group: the child it runs in (None: in process);
    switches: the inventory rows it covers (default: the names of env); taken: what its evidence must say"""
    env = dict(env or {})
    c = Case(name, fn, env, tuple(switches if switches is not None else env), group, taken)
    table = INPROC if group is None else CHILD
    assert name not in INPROC and name not in CHILD, name
    table[name] = c
    return c


def referenced_switches():
    """every inventory row some case covers"""
    out = set()
    for c in list(INPROC.values()) + list(CHILD.values()):
        out.update(c.switches)
    return out


DEVICE_ERROR = re.compile(r"HIP error|hipError|HIP runtime error|illegal memory access|[Mm]emory access fault|accelerator|HSA_STATUS|device-side assert|"
                          r"unspecified launch failure|hardware exception", re.I)


def device_error(e):
    """an MI355_ERR_HIP of the library, or a torch / runtime error whose text names the device (an asynchronous fault surfaces at a later
    synchronize or copy as a RuntimeError)"""
    return getattr(e, "code", 0) == -4 or bool(DEVICE_ERROR.search("%s: %s" % (type(e).__name__, e)))


def install_log(pkg):
    del LOG[:]
    pkg.set_log_callback(lambda level, msg: LOG.append(msg))


def noted(name):
    """the once-per-process line of a launch-time switch"""
    for line in LOG:
        if line.startswith("switch %s:" % name):
            return line
    return None


def said(prefix, mark=0):
    """the last INFO line since `mark` that starts with prefix ('' if none)"""
    for line in reversed(LOG[mark:]):
        if line.startswith(prefix):
            return line
    return ""


def relerr(got, ref):
    from conftest import relerr as r
    return r(got, ref)


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def bits_differ(a, b):
    """0.0 when two arrays are equal bit for bit, 1.0 otherwise (bound 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return 0.0 if a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) else 1.0


def result(taken, evidence, checks):
    return {"taken": taken, "evidence": evidence or "", "checks": [[str(l), float(e), float(b)] for l, e, b in checks]}


# ------------------------------------------------------------------------------------------------------------------------ clFFT

MODES = {"fwd_shift_win": (True, True, True, False), "bwd_shift": (False, True, False, False), "fwd": (True, False, False, False),
         "bwd_win": (False, False, True, False), "real_fwd_shift_win": (True, True, True, True)}
SMALL = list(MODES)  # the modes of SMALL in tests/test_device_bounds_gpu.py


def fft_bound(n):
    """2e-6 for a power of two, 3e-6 for a 2-3-5-7-11-13 length (what tests/test_fft_gpu.py asks of the default routes), else the budget"""
    if n & (n - 1) == 0:
        return 2e-6
    m = n
    for p in (2, 3, 5, 7, 11, 13):
        while m % p == 0:
            m //= p
    return 3e-6 if m == 1 else TOL


def fft_used(blk, got, n, fwd, w, shift, x):
    """the largest used fraction of the per-bin and per-frame bounds of tests/fft_ref.py (bound 1.0), with the multiples of the route blk's last
    call took; a zero frame that did not come out as zeros counts as inf (fft_bound_check returns that)"""
    from fft_ref import fft_bound_check, fft_bound_kind, fft_frames64
    x = np.asarray(x)
    return max(fft_bound_check(got, fft_frames64(n, fwd, w, shift, x, not np.iscomplexobj(x)), n, fft_bound_kind(blk.last_route()), check=False))


def run_fft(pkg, oracle, n, frames, mode, pick=None):
    """device path, NaN-filled output; every frame (or the frames of `pick`) against numpy's float64 FFT: the largest relerr of a batch,
    and the largest used fraction of the per-bin and per-frame bounds (tests/fft_ref.py, the multiples of the route that ran; bound 1.0)"""
    import torch
    from fft_ref import np_fft_block as _np_fft_block
    fwd, shift, win, real = MODES[mode]
    w = oracle.window(oracle.WIN_BLACKMAN_HARRIS, n) if win else None
    blk = pkg.clFFT(n, pkg.CLFFT_FORWARD if fwd else pkg.CLFFT_BACKWARD, [] if w is None else w, pkg.DTYPE_FLOAT if real else pkg.DTYPE_COMPLEX,
                    *GPU_ARGS, 1, 1, shift)
    k = 1 if real else 2
    g = torch.Generator(device="cuda").manual_seed(n * 31 + frames)
    x = torch.randn(frames * n * k, device="cuda", generator=g)
    y = torch.full((frames * n * 2,), float("nan"), device="cuda")
    blk.work_device(frames, [x], [y])
    torch.cuda.synchronize()
    want = sorted(set(range(frames) if pick is None else pick))
    per = max(1, (1 << 21) // n)  # frames per compared batch
    runs, i = [], 0
    while i < len(want):
        j = i
        while j + 1 < len(want) and want[j + 1] == want[j] + 1 and j + 1 - i < per:
            j += 1
        runs.append((want[i], want[j] + 1))
        i = j + 1
    errs, used = [], []
    for f0, f1 in runs:
        xs = x[f0 * n * k:f1 * n * k].cpu().numpy()
        xs = xs if real else xs.view(np.complex64)
        got = y[f0 * n * 2:f1 * n * 2].cpu().numpy().view(np.complex64)
        errs.append(relerr(got, _np_fft_block(n, fwd, w, shift, xs)))
        used.append(fft_used(blk, got, n, fwd, w, shift, xs))
    blk.stop()
    return float(np.max(np.array(errs))), float(np.max(np.array(used)))


def fft_case(name, shapes, env=None, group=None, note=None, plan=None, switches=None, taken=True, modes=SMALL, pick=None, bound=fft_bound):
    """a clFFT case: evidence is the once-per-process line of `note`, or `plan` in the INFO line of create"""
    def fn(pkg, oracle):
        checks = []
        ev, tk = "", None
        for n, fr in shapes:
            for m in modes:
                m0 = len(LOG)
                err, used = run_fft(pkg, oracle, n, fr, m, pick and pick(fr))
                checks.append(("clFFT %d x %d %s" % (n, fr, m), err, bound(n)))
                checks.append(("clFFT %d x %d %s: per-bin / per-frame bounds used" % (n, fr, m), used, 1.0))
                if plan:
                    line = said("clFFT: %d points" % n, m0)
                    ok = line.endswith(": " + plan)
                    tk = ok if tk is None else (tk and ok)
                    ev = line
        if note:
            ev = noted(note)
            tk = ev is not None
        return result(tk, ev, checks)
    return add(name, fn, env, group, switches, taken)


def six(frames):
    """the first frame, the frames either side of both piece boundaries, the last (pieces of (frames - 3) / 2)"""
    p = (frames - 3) // 2
    return [0, p - 1, p, 2 * p - 1, 2 * p, frames - 1]


GROUPS["fft_routes"] = {"MI355_FFT_WAVE_GEO": "1", "MI355_FFT_WHOLE_FRAME": "1"}
fft_case("fft_wave_geo", [(n, 3 * 4096 // n + 1) for n in (16, 64, 256, 1024)], group="fft_routes", note="MI355_FFT_WAVE_GEO",
         switches=["MI355_FFT_WAVE_GEO"])
fft_case("fft_whole_frame", [(8192, 5), (16384, 5)], group="fft_routes", note="MI355_FFT_WHOLE_FRAME", switches=["MI355_FFT_WHOLE_FRAME"])
fft_case("fft_32768_in_registers", [(32768, 3)], {"MI355_FFT_32768_IN_REGISTERS": "1"}, group="fft_routes", note="MI355_FFT_32768_IN_REGISTERS")
fft_case("fft_32768_two_kernels", [(32768, 3)], {"MI355_FFT_32768_TWO_KERNELS": "1"}, plan="multi-pass")
fft_case("fft_no_tile", [(65536, 2), (131072, 2), (1048576, 2)], {"MI355_FFT_NO_TILE": "1"}, plan="multi-pass")
for _n1 in (256, 512, 1024):
    for _wr in ("0", "1"):
        fft_case("fft_tile_n1_%d_wreg_%s" % (_n1, _wr), [(1 << 18, 2)], {"MI355_FFT_TILE_N1": str(_n1), "MI355_FFT_TILE_WREG": _wr}, taken=None)
GROUPS["fft_tile_half"] = {"MI355_FFT_TILE_HALF": "0"}
fft_case("fft_tile_half", [(1 << 19, 2), (1 << 20, 2)], group="fft_tile_half", note="MI355_FFT_TILE_HALF", switches=["MI355_FFT_TILE_HALF"])
GROUPS["chirpz"] = {"MI355_CHIRPZ_FUSED": "0"}
fft_case("chirpz_unfused", [(131, 7), (1201, 7), (4099, 7)], group="chirpz", note="MI355_CHIRPZ_FUSED", switches=["MI355_CHIRPZ_FUSED"])
# 128 MiB / (16384 x 8 B) = 1024 frames per piece of the five-launch path
fft_case("chirpz_unfused_three_pieces", [(4099, 2 * 1024 + 3)], group="chirpz", note="MI355_CHIRPZ_FUSED", switches=["MI355_CHIRPZ_FUSED"],
         modes=["fwd"])
# m = 65536 is the five-launch path by default: 256 frames per piece
fft_case("chirpz_16385_three_pieces", [(16385, 2 * 256 + 3)], switches=[], taken=None, modes=["fwd_shift_win"], pick=six)
GROUPS["fft_mr_no_copy"] = {"MI355_FFT_MR_NO_COPY_OUT": "1"}
GROUPS["fft_mr_runs"] = {"MI355_FFT_MR_COPY_OUT_NS": "0", "MI355_FFT_MR_COPY_IN_NB": "0"}
_MR = [(n, 11) for n in (6, 12, 48, 100, 200, 1000)]
fft_case("fft_mr_no_copy_out", _MR, group="fft_mr_no_copy", note="MI355_FFT_MR_NO_COPY_OUT", switches=["MI355_FFT_MR_NO_COPY_OUT"])
fft_case("fft_mr_copy_out_ns", _MR, group="fft_mr_runs", note="MI355_FFT_MR_COPY_OUT_NS", switches=["MI355_FFT_MR_COPY_OUT_NS"])
fft_case("fft_mr_copy_in_nb", _MR, group="fft_mr_runs", note="MI355_FFT_MR_COPY_IN_NB", switches=["MI355_FFT_MR_COPY_IN_NB"])
# workspace pieces of 1 MiB: 65536 points = 2 frames per piece, 131072 = 1, 2^21 = 1 (never less than a frame)
GROUPS["fft_ws"] = {"MI355_FFT_WS_MB": "1"}
fft_case("fft_ws_tile_route", [(65536, 5)], group="fft_ws", note="MI355_FFT_WS_MB", switches=["MI355_FFT_WS_MB"])
fft_case("fft_ws_no_tile", [(65536, 3), (131072, 3)], {"MI355_FFT_NO_TILE": "1"}, group="fft_ws", note="MI355_FFT_WS_MB",
         switches=["MI355_FFT_WS_MB", "MI355_FFT_NO_TILE"])
fft_case("fft_ws_four_passes", [(1 << 21, 2)], group="fft_ws", note="MI355_FFT_WS_MB", switches=["MI355_FFT_WS_MB"], modes=["fwd_shift_win", "bwd_shift"])
# tuning and reroute rows of the block
fft_case("fft_wg_per_cu", [(1024, 3 * 256 * 4 + 5)], {"MI355_FFT_WG_PER_CU": "1"}, taken=None, modes=["fwd_shift_win", "bwd_win"])
fft_case("wg_per_cu", [(8192, 300)], {"MI355_WG_PER_CU": "1"}, taken=None, modes=["fwd_shift_win"])
for _p in ("0", "1", "2"):
    # (a persistent-sized call, 16 groups per CU and a ragged end: the size at which the three forms are used)
    fft_case("fft_prefetch_%s" % _p, [(4096, 256 * 16 + 37)], {"MI355_FFT_PREFETCH": _p}, taken=None, modes=["fwd_shift_win", "real_fwd_shift_win"])
fft_case("fft_no_mr", [(1200, 7)], {"MI355_FFT_NO_MR": "1"}, plan="chirp-z over a power-of-two transform")
for _v in ("0", "1"):
    fft_case("fft_mr_variant_%s" % _v, [(96, 11)], {"MI355_FFT_MR_VARIANT": _v}, taken=None)
fft_case("fft_mr_rule", [(675, 11)], {"MI355_FFT_MR_AUTOTUNE": "0"}, taken=None)
fft_case("fft_mr_timed_variant", [(2400, 5)], {"MI355_FFT_MR_TIMED_VARIANT": "1"}, taken=None)
fft_case("fft_mr_threads_frames", [(120, 1000)], {"MI355_FFT_MR_THREADS": "64", "MI355_FFT_MR_FRAMES": "1", "MI355_FFT_MR_AUTOTUNE": "0"},
         taken=None, switches=["MI355_FFT_MR_THREADS", "MI355_FFT_MR_FRAMES"])


def _fft_sched(pkg, oracle):
    """MI355_FFT_SCHED: claims and static stride give the same bits (a persistent-sized call: two workgroups per CU with 8 groups each)"""
    import torch
    n = 4096
    frames = torch.cuda.get_device_properties(0).multi_processor_count * 16 + 37
    blk = pkg.clFFT(n, pkg.CLFFT_FORWARD, [], pkg.DTYPE_COMPLEX, *GPU_ARGS, 1, 1, True)
    x = torch.randn(frames * n * 2, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    outs = []
    for s in ("1", "0"):
        os.environ["MI355_FFT_SCHED"] = s
        y = torch.full((frames * n * 2,), float("nan"), device="cuda")
        blk.work_device(frames, [x], [y])
        torch.cuda.synchronize()
        outs.append(y)
    from fft_ref import np_fft_block as _np_fft_block
    f0 = frames - 64
    ref = _np_fft_block(n, True, None, True, x[f0 * n * 2:].cpu().numpy().view(np.complex64))
    got = outs[1][f0 * n * 2:].cpu().numpy().view(np.complex64)
    err = relerr(got, ref)
    used = fft_used(blk, got, n, True, None, True, x[f0 * n * 2:].cpu().numpy().view(np.complex64))
    return result(None, "", [("static stride, last 64 frames", err, 2e-6), ("static stride, last 64 frames: per-bin / per-frame bounds used", used, 1.0), ("claims == static stride", 0.0 if torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) else 1.0, 0.0)])


add("fft_sched", _fft_sched, {"MI355_FFT_SCHED": "0"}, taken=None)


# ---------------------------------------------------------------------------------------------------------------------- filters

def conv64(x, t):
    """full convolution in float64 through numpy's FFT (error ~ 1e-15 of the largest product sum)"""
    n = x.size + t.size - 1
    nf = 1 << int(n - 1).bit_length()
    return np.fft.ifft(np.fft.fft(x.astype(np.complex128), nf) * np.fft.fft(t.astype(np.complex128), nf))[:n]


def run_fir(pkg, ntaps, decim, ctaps, use_time, nout):
    """device path on a NaN-filled output, history-prefixed random input (the history is not zero); float64 reference"""
    import torch
    rng = np.random.default_rng(ntaps * 13 + decim + (1 if ctaps else 0))
    if ctaps:
        taps = (crandn(rng, ntaps) / np.sqrt(ntaps)).astype(np.complex64)
        blk = pkg.clComplexFilter(*GPU_ARGS, decim, taps, 1, 1, use_time=use_time)
    else:
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        blk = pkg.clFilter(*GPU_ARGS, decim, taps, 1, 1, use_time)
    xh = crandn(rng, nout * decim + ntaps - 1)
    y = torch.full((nout,), float("nan"), dtype=torch.complex64, device="cuda")
    blk.work_device(nout, [torch.from_numpy(xh).cuda()], [y])
    torch.cuda.synchronize()
    ref = conv64(xh, taps)[ntaps - 1::decim][:nout]
    blk.stop()
    return relerr(y.cpu().numpy(), ref)


def fir_case(name, shapes, env=None, group=None, note=None, switches=None, taken=True, use_time=True, created=None):
    """shapes: (ntaps, decim, complex taps, outputs); evidence: the once-per-process line of `note`, or `created` in every INFO line of create"""
    def fn(pkg, oracle):
        m0 = len(LOG)
        checks = [("%s %d %s taps decim %d x %d" % ("direct form" if use_time else "overlap-save", nt, "complex" if ct else "real", d, nout),
                   run_fir(pkg, nt, d, ct, use_time, nout), TOL) for nt, d, ct, nout in shapes]
        if created:
            lines = [l for l in LOG[m0:] if l.startswith(("clFilter:", "clComplexFilter:"))]
            return result(len(lines) == len(shapes) and all(created in l for l in lines), " | ".join(lines), checks)
        ev = noted(note) if note else ""
        return result((ev is not None) if note else None, ev, checks)
    return add(name, fn, env, group, switches, taken)


GROUPS["filter_mfma"] = {"MI355_FIR_MFMA": "0"}
GROUPS["filter_tune"] = {"MI355_FIR_DEC_LDS_MIN": "12", "MI355_FIR_DEC2_SPAN": "2048"}
fir_case("fir_mfma_off", [(nt, d, False, 5000 + nt) for nt in (16, 65, 129, 1000, 9000) for d in (1, 2, 8)] +
         [(nt, d, True, 5000 + nt) for nt in (65, 1500) for d in (1, 2, 8)], group="filter_mfma", note="MI355_FIR_MFMA", switches=["MI355_FIR_MFMA"])
_DEC = [(65, 16, False), (65, 9, False), (77, 15, True), (200, 25, False), (33, 33, False), (129, 10, True), (1000, 21, False)]  # test_lds_staged_decimators_agree
_DECS = [(nt, d, ct, 40000 + 13) for nt, d, ct in _DEC]
# decimations 9 ... 11 change sides with the bound at 12: fewer than 16 taps leave the register-tiled kernel (k_fir_td) for the decimating ones, and
# with every output asked for (MI355_FIR_DEC_KERNEL=all) 65 and 129 taps leave k_fir_mfma; decimation 12 and 16 stay where they were
fir_case("fir_dec_lds_min_few_taps", [(9, d, ct, 40013) for d in (9, 10, 11, 12) for ct in (False, True)], group="filter_tune", note="MI355_FIR_DEC_LDS_MIN",
         switches=["MI355_FIR_DEC_LDS_MIN"])
fir_case("fir_dec_lds_min_all_outputs", [(65, 10, False, 40013), (129, 11, True, 40013), (65, 16, False, 40013)], {"MI355_FIR_DEC_KERNEL": "all"},
         group="filter_tune", note="MI355_FIR_DEC_LDS_MIN", switches=["MI355_FIR_DEC_LDS_MIN"])
fir_case("fir_dec_lds_min", _DECS, group="filter_tune", switches=["MI355_FIR_DEC_LDS_MIN"], taken=None)
fir_case("fir_dec2_span", _DECS, {"MI355_FIR_DEC_KERNEL": "lds"}, group="filter_tune", note="MI355_FIR_DEC2_SPAN",
         switches=["MI355_FIR_DEC2_SPAN", "MI355_FIR_DEC_KERNEL"])
# (each of the two once-per-process switches of launch_ols_g in a child of its own: the segment loop with the default, 16-aligned blocks is what
# MI355_OLS_PART_ONE_PASS=0 gives a user)
GROUPS["filter_part"] = {"MI355_OLS_PART_ONE_PASS": "0"}
GROUPS["filter_align"] = {"MI355_OLS_ALIGN": "0"}
fir_case("fir_dec_lds_off", _DECS, {"MI355_FIR_DEC_LDS_OFF": "1"}, group="filter_part", note="MI355_FIR_DEC_LDS_OFF")
fir_case("fir_dec2_even_only", _DECS, {"MI355_FIR_DEC2_EVEN_ONLY": "1", "MI355_FIR_DEC_KERNEL": "lds"}, group="filter_part", note="MI355_FIR_DEC2_EVEN_ONLY",
         switches=["MI355_FIR_DEC2_EVEN_ONLY"])
# (the switch acts on decimations 3 ... 5 only: two such shapes beside the ones of test_lds_staged_decimators_agree)
fir_case("fir_dec2_from_6", _DECS + [(65, 4, False, 40013), (200, 5, True, 40013)], {"MI355_FIR_DEC2_FROM_6": "1"}, group="filter_part",
         note="MI355_FIR_DEC2_FROM_6")
# (2049 ... 10240 taps run k_ols_ups unless MI355_OLS_UPS=0: the segment loop, and its line, belong to the second case)
fir_case("ols_part_switch_with_ups", [(nt, d, ct, 20000) for nt in (5000, 9000) for d in (1, 3) for ct in (False, True)], group="filter_part",
         switches=[], taken=None, use_time=False)
fir_case("ols_part_segments", [(nt, d, ct, 20000) for nt in (5000, 9000) for d in (1, 3) for ct in (False, True)], {"MI355_OLS_UPS": "0"}, group="filter_part",
         note="MI355_OLS_PART_ONE_PASS", switches=["MI355_OLS_PART_ONE_PASS", "MI355_OLS_UPS"], use_time=False)
fir_case("ols_unaligned", [(nt, d, ct, 20000) for nt in (3, 65, 2048) for d, ct in ((1, False), (2, True))], group="filter_align", note="MI355_OLS_ALIGN",
         switches=["MI355_OLS_ALIGN"], use_time=False)
fir_case("ols_unaligned_ragged", [(nt, d, ct, 20000) for nt in (3, 65, 2048) for d, ct in ((1, False), (2, True))], {"MI355_OLS_RAGGED_L": "1"},
         group="filter_align", note="MI355_OLS_RAGGED_L", use_time=False)
fir_case("ols_xcd_map", [(65, 1, False, 20000), (65, 3, True, 20000)], {"MI355_OLS_XCD_MAP": "1"}, group="filter_mfma", note="MI355_OLS_XCD_MAP", use_time=False)
fir_case("ols_part_plain_order", [(5000, 1, False, 20000), (5000, 3, True, 20000)], {"MI355_OLS_PART_XCD_MAP": "0", "MI355_OLS_UPS": "0"}, group="filter_mfma",
         note="MI355_OLS_PART_XCD_MAP", switches=["MI355_OLS_PART_XCD_MAP"], use_time=False)
# tuning and reroute rows: one workgroup per CU makes the grid-stride loops run many iterations
fir_case("td_wg_per_cu", [(9, 1, False, 2048 * 300 + 5), (65, 1, False, 4096 * 300 + 5)], {"MI355_TD_WG_PER_CU": "1"}, taken=None)
fir_case("ols_ups_wgs", [(5000, 1, False, 2048 * 40 + 77)], {"MI355_OLS_UPS_WGS": "3"}, taken=None, use_time=False)
fir_case("filter_fft_wave_geo", [(30, 1, False, 20000), (30, 3, True, 20000)], {"MI355_FILTER_FFT": "512", "MI355_FILTER_WAVE_GEO": "1"}, use_time=False,
         created="(transform size 512)")  # (30 taps choose 256 by themselves)
fir_case("fir_dec2_off_pad", [(65, 16, False, 40013)], {"MI355_FIR_DEC_KERNEL": "lds", "MI355_FIR_DEC2_PAD": "1"}, taken=None,
         switches=["MI355_FIR_DEC2_PAD", "MI355_FIR_DEC_KERNEL"])
fir_case("fir_dec2_off", [(65, 16, False, 40013)], {"MI355_FIR_DEC_KERNEL": "lds", "MI355_FIR_DEC2_OFF": "1"}, taken=None, switches=["MI355_FIR_DEC2_OFF"])


def fir_window_case(name, shapes, route, group, switches):
    """every component of every output within the per-output bound of tests/fir_ref.py (error / bound against 1.0), on the kernel `route`
    names: evidence is last_route() of every shape.  shapes: (ntaps, decim, complex taps); two tiles of the kernel and a ragged third."""
    def fn(pkg, oracle):
        import fir_ref
        import torch
        checks, routes = [], []
        for K, D, ct in shapes:
            n = fir_ref.nout(route.split("<")[0], K, D)
            h, x = fir_ref.make_taps(K, ct), fir_ref.make_input(K, D, n)
            blk = (pkg.clComplexFilter if ct else pkg.clFilter)(*GPU_ARGS, D, h, 1, 1, True)
            y = torch.full((n,), float("nan"), dtype=torch.complex64, device="cuda")
            blk.work_device(n, [torch.from_numpy(x).cuda()], [y])
            torch.cuda.synchronize()
            routes.append(blk.last_route())
            checks.append(("%s %d taps decim %d x %d, error / bound per output" % (routes[-1], K, D, n),
                           fir_ref.worst(y.cpu().numpy(), fir_ref.fir(h, x, D, n), fir_ref.bound(h, x, D, n)), 1.0))
            blk.stop()
        return result(all(r == route for r in routes), " | ".join(routes), checks)
    return add(name, fn, None, group, switches)


# k_fir_td with 16 taps and more runs only with the matrix-core kernel switched off (read once per process)
fir_window_case("fir_td_window_mfma_off", [(K, D, False) for K in (16, 65, 129) for D in (1, 2)], "k_fir_td<real>", "filter_mfma", ["MI355_FIR_MFMA"])


# ------------------------------------------------------------------------------------------------------------------ channelizer

def run_pfb(pkg, oracle, M, R, per_arm, steps, nmap=None):
    import torch
    nmap = M if nmap is None else nmap
    rng = np.random.default_rng(M * 17 + R + per_arm + nmap)
    K = M * per_arm - (M // 3 if per_arm % 2 and per_arm > 1 else 0)  # ragged last arm for the odd tap counts
    taps = (rng.standard_normal(K) / np.sqrt(per_arm)).astype(np.float32)
    buf = steps * R
    while buf % M:
        steps += 1
        buf = steps * R
    chmap = list(range(M)) if nmap == M else rng.permutation(M)[:nmap].tolist()
    blk = pkg.clPolyphaseChannelizer(*GPU_ARGS, taps, buf, M, R, chmap, 1)
    xh = crandn(rng, blk.ninput())
    y = torch.full((blk.noutput(),), float("nan"), dtype=torch.complex64, device="cuda")
    blk.work_device([torch.from_numpy(xh).cuda()], [y])
    torch.cuda.synchronize()
    ref = oracle.pfb(taps, buf, M, R, chmap, xh, f64=True)
    blk.stop()
    return relerr(y.cpu().numpy(), ref)


def pfb_case(name, shapes, env=None, group=None, note=None, kernel=None, switches=None, taken=True):
    """shapes: (channels, inputs per step, taps per arm, steps); kernel: what create's INFO line must end with"""
    def fn(pkg, oracle):
        checks, tk, ev = [], None, ""
        for M, R, pa, st in shapes:
            m0 = len(LOG)
            checks.append(("channelizer %d ch R %d, %d taps per arm, %d steps" % (M, R, pa, st), run_pfb(pkg, oracle, M, R, pa, st), TOL))
            if kernel:
                ev = said("clPolyphaseChannelizer:", m0)
                tk = ev.endswith(kernel) if tk is None else (tk and ev.endswith(kernel))
        if note:
            ev = noted(note)
            tk = ev is not None
        return result(tk, ev, checks)
    return add(name, fn, env, group, switches, taken)


GROUPS["pfb"] = {"MI355_PFB_WAVE": "0", "MI355_PFB_NO_XCD_RUNS": "1", "MI355_PFB_MR_THREADS": "256", "MI355_PFB_MR_WG_PER_CU": "1"}
# 4096 / M steps per workgroup iteration of the staged kernel: three iterations and a ragged end
# (2 and 8 channels, and 33 taps per arm, are the staged kernel's anyway; k_pfb<32>, <64>, <128> and <256> run with the switch only)
pfb_case("pfb_staged", [(M, M, pa, 3 * (4096 // M) + 37) for M in (2, 8, 64) for pa in (1, 8, 33)] +
         [(M, M, pa, 3 * (4096 // M) + 37) for M in (32, 128, 256) for pa in (1, 8, 32)], group="pfb", note="MI355_PFB_WAVE", switches=["MI355_PFB_WAVE"])
# (512 channels have no staged kernel: with the switch set they are created on the two-kernel form)
pfb_case("pfb_staged_512", [(512, 512, pa, 61) for pa in (1, 8, 33)], group="pfb", kernel="two-pass kernel", switches=["MI355_PFB_WAVE"])
pfb_case("pfb_no_xcd_runs", [(1024, 1024, 32, 300), (600, 600, 25, 100)], {"MI355_PFB_NO_FIR_RING": "1"}, group="pfb", note="MI355_PFB_NO_XCD_RUNS",
         switches=["MI355_PFB_NO_XCD_RUNS"])
pfb_case("pfb_mr_threads", [(100, 100, 32, 70 * 40 + 3), (12, 12, 7, 5000)], group="pfb", note="MI355_PFB_MR_THREADS",
         switches=["MI355_PFB_MR_THREADS", "MI355_PFB_MR_WG_PER_CU"])
pfb_case("pfb_no_ring_512", [(512, 512, 8, 61), (512, 512, 32, 61)], {"MI355_PFB_NO_RING_512": "1"}, kernel="two-pass kernel")
pfb_case("pfb_waves_per_cu", [(64, 64, 32, 16 * 3000 + 5), (512, 512, 8, 16 * 300 + 5)], {"MI355_PFB_WAVES_PER_CU": "1", "MI355_PFB_SMALL": "0"}, taken=None)
pfb_case("pfb_small_off", [(64, 64, 8, 101), (16, 16, 32, 293)], {"MI355_PFB_SMALL": "0"}, taken=None)
pfb_case("pfb_no_fir_ring", [(1024, 1024, 32, 45), (1000, 1000, 7, 83)], {"MI355_PFB_NO_FIR_RING": "1"}, taken=None)
pfb_case("pfb_branches_per_output", [(1024, 1024, 32, 45), (128, 32, 32, 134)], {"MI355_PFB_BRANCHES_PER_OUTPUT": "1", "MI355_PFB_NO_FAST_OVERSAMPLED": "1"}, taken=None)
pfb_case("pfb_no_fast_oversampled", [(64, 32, 8, 203), (128, 32, 32, 134)], {"MI355_PFB_NO_FAST_OVERSAMPLED": "1"}, kernel="two-pass kernel")
pfb_case("pfb_no_mr_fused", [(100, 100, 32, 70)], {"MI355_PFB_NO_MR_FUSED": "1"}, taken=None)
pfb_case("pfb_direct_dft", [(100, 30, 5, 83), (1000, 1000, 7, 83)], {"MI355_PFB_DIRECT_DFT": "1"}, taken=None)


def pfb_window_case(name, shapes, group, switches):
    """the same for the channelizer and the per-step bound of tests/pfb_ref.py; shapes: (channels, inputs per step, taps per arm, steps,
    the first kernel last_route() must name); identity map and one that repeats and omits channels"""
    def fn(pkg, oracle):
        import pfb_ref
        import torch
        checks, routes, tk = [], [], True
        for M, R, P, steps, first in shapes:
            h = pfb_ref.make_taps(M, P)
            x = pfb_ref.make_input(h.size, R, steps)
            for cm in pfb_ref.maps(M):
                blk = pkg.clPolyphaseChannelizer(*GPU_ARGS, h, steps * R, M, R, cm, 1)
                y = torch.full((blk.noutput(),), float("nan"), dtype=torch.complex64, device="cuda")
                blk.work_device([torch.from_numpy(x).cuda()], [y])
                torch.cuda.synchronize()
                routes.append(blk.last_route())
                tk = tk and routes[-1].split(" + ")[0] == first
                want, bnd = pfb_ref.channelize(h, M, R, cm, x, steps)
                checks.append(("%s %d / %d, %d taps per arm, %d mapped x %d steps, error / bound per step" % (routes[-1], M, R, P, len(cm), steps),
                               pfb_ref.worst(y.cpu().numpy(), want, bnd, len(cm)), 1.0))
                blk.stop()
        return result(tk, " | ".join(routes), checks)
    return add(name, fn, None, group, switches)


# the staged kernel k_pfb<M, PMAX> at the channel counts the wave kernels take otherwise: 4096 / M steps per workgroup iteration, two and a ragged third
pfb_window_case("pfb_staged_window", [(32, 32, 8, 2 * 128 + 37, "k_pfb<32,8>"), (64, 64, 32, 2 * 64 + 37, "k_pfb<64,32>"), (256, 256, 5, 2 * 16 + 37, "k_pfb<256,8>")],
                "pfb", ["MI355_PFB_WAVE"])


# ------------------------------------------------------------------------------------------------------- resampler, synthesizer

def _resampler(name, kernel):
    def fn(pkg, oracle):
        """bit-identical to the default kernel (resample.hip: 'any of the kernels give the same bits') and within the yardstick's bound"""
        import torch
        import resampler_ref as ref
        checks, tk, ev = [], True, ""
        for L, M, K in ((8, 1, 89), (2, 1, 65), (3, 2, 97), (160, 147, 3840)):
            for cplx in (False, True):
                h = ref.make_taps(K, cplx)
                os.environ.pop(name, None)
                m0 = len(LOG)
                dflt = pkg.clRationalResampler(*GPU_ARGS, L, M, h, 1)
                line = said("clRationalResampler:", m0)
                tile = re.search(r"tiles of (\d+) outputs", line)
                n = 3 * (int(tile.group(1)) if tile else 256) + 5  # (k_rs_interp: tiles of 256 input samples)
                os.environ[name] = "1"
                m0 = len(LOG)
                blk = pkg.clRationalResampler(*GPU_ARGS, L, M, h, 1)
                ev = said("clRationalResampler:", m0)
                # GENERAL only acts where the interpolation kernel would serve
                acts = kernel != "k_rs_lds" or "k_rs_interp" in line
                tk = tk and ((kernel in ev) if acts else (ev.split(":", 1)[1] == line.split(":", 1)[1]))
                c = L // 2
                x = ref.make_input(L, M, K, c, n)
                outs = []
                for b in (dflt, blk):
                    y = torch.full((n,), float("nan"), dtype=torch.complex64, device="cuda")
                    b.set_phase(c)
                    b.work_device(n, [torch.from_numpy(x).cuda()], [y])
                    torch.cuda.synchronize()
                    outs.append(y.cpu().numpy())
                    b.stop()
                tag = "resampler %d/%d %d %s taps x %d" % (L, M, K, "complex" if cplx else "real", n)
                checks.append((tag + " error / bound", ref.worst(outs[1], ref.resample(h, L, M, x, n, c)[0], ref.bound(h, L, x, c, M, n)), 1.0))
                checks.append((tag + " bits", bits_differ(outs[0], outs[1]), 0.0))
        return result(tk, ev, checks)
    return fn


for _name, _k in (("MI355_RESAMPLER_PLAIN", "k_rs_plain"), ("MI355_RESAMPLER_GENERAL", "k_rs_lds")):
    add(_name[6:].lower(), _resampler(_name, _k), {_name: "1"})


def _synth(name, want):
    def fn(pkg, oracle):
        import torch
        import synth_ref as ref
        checks, tk, ev = [], True, ""
        for M, T in ((64, 8), (4096, 5), (12, 4)):
            g = ref.make_taps(T * M - 1)
            blk = pkg.clPolyphaseSynthesizer(*GPU_ARGS, g, M, None, 1)
            ev = blk.route()
            m = re.search(r"tile=(\d+)", ev)
            # (MI355_SYNTH_TAPS_GLOBAL acts where the power-of-two route's taps fit the LDS beside the ring: 64 channels x 8 taps do, 4096 x 5 do
            # not, 12 channels run the mixed-radix route; the generic route has no tile: 16 frames stand in)
            acts = name != "MI355_SYNTH_TAPS_GLOBAL" or (M, T) == (64, 8)
            tk = tk and ((want in ev) if acts else True)
            n = 3 * (int(m.group(1)) if m else 16) + 5
            x = ref.make_input(g.size, M, M, n)
            y = torch.full((n * M,), float("nan"), dtype=torch.complex64, device="cuda")
            blk.work_device(n, [torch.from_numpy(x).cuda()], [y])
            torch.cuda.synchronize()
            checks.append(("synthesizer %d ch, %d taps per arm, %d frames (%s)" % (M, T, n, ev), relerr(y.cpu().numpy(), ref.synth(g, M, None, x, n).astype(np.complex64)), ref.TOL))
            blk.stop()
            if name == "MI355_SYNTH_TAPS_GLOBAL":  # "comparison variants, same bits" (include/mi355_clenabled.h)
                os.environ.pop(name)
                dflt = pkg.clPolyphaseSynthesizer(*GPU_ARGS, g, M, None, 1)
                os.environ[name] = "1"
                y0 = torch.full((n * M,), float("nan"), dtype=torch.complex64, device="cuda")
                dflt.work_device(n, [torch.from_numpy(x).cuda()], [y0])
                torch.cuda.synchronize()
                checks.append(("synthesizer %d ch: bits of the default (%s)" % (M, dflt.route()), bits_differ(y.cpu().numpy(), y0.cpu().numpy()), 0.0))
                tk = tk and "taps=global" not in dflt.route()
                dflt.stop()
        return result(tk, ev, checks)
    return add(name[6:].lower(), fn, {name: "1"})


_synth("MI355_SYNTH_TAPS_GLOBAL", "taps=global")
_synth("MI355_SYNTH_GENERIC", "generic")


def _loops(pkg, oracle):
    """the comparison variants of clSignalSource / clCostasLoop, named by create's INFO line, against the float64 yardstick (tests/loops_ref.py) with
    the tolerances of tests/test_loops_gpu.py: 2^-22 of the amplitude per component, 1e-5 of the largest input / of a radian per sample"""
    import torch
    import loops_ref as ref
    n = 4097
    m0 = len(LOG)
    src = pkg.clSignalSource(1, *GPU_ARGS, 48000.0, 1, 1234.5, 1.0, 1)
    loop = pkg.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, 4, 1)
    text = " | ".join(LOG[m0:])
    comp = lambda got, want: max(np.abs(got.real.astype(np.float64) - want.real).max(), np.abs(got.imag.astype(np.float64) - want.imag).max())  # noqa: E731
    y = torch.full((n,), float("nan"), dtype=torch.complex64, device="cuda")
    src.work_device(n, [], [y])
    want_s, _ = ref.sig_call(0.0, ref.sig_inc(1234.5, 48000.0), n, 1.0, "complex", 1)
    x, _ = ref.costas_input(4, 1, n)
    want, want_f, _ = ref.costas_expected(4, 1, n)
    out = torch.full((n,), float("nan"), dtype=torch.complex64, device="cuda")
    freq = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    loop.work_device(n, [torch.from_numpy(x).cuda()], [out, freq])
    torch.cuda.synchronize()
    checks = [("clSignalSource, one sincos per item", comp(y.cpu().numpy(), want_s), 2.0 ** -22),
              ("clCostasLoop as one lane, output", comp(out.cpu().numpy(), want) / float(np.abs(x).max()), 1e-5),
              ("clCostasLoop as one lane, frequency", float(np.abs(freq.cpu().numpy().astype(np.float64) - want_f).max()), 1e-5)]
    return result("literal" in text and "k_costas_lanes" in text, text, checks)


add("loops_variants", _loops, {"MI355_SIGSOURCE_LITERAL": "1", "MI355_COSTAS_ONE_LANE": "1"})


# ------------------------------------------------------------------------------------------------------------------- host paths

def _host_small(pkg, oracle):
    """8192 items through work() of clMathOp, clFFT 1024, clFilter (65 taps, decimation 2) and clComplexToMagPhase"""
    rng = np.random.default_rng(11)
    n = 8192
    checks = []
    a, b = crandn(rng, n), crandn(rng, n)
    c = np.full(n, np.nan, np.complex64)
    pkg.clMathOp(pkg.DTYPE_COMPLEX, *GPU_ARGS, pkg.MATHOP_MULTIPLY, 1).work(n, [a, b], [c])
    checks.append(("clMathOp multiply 8192", relerr(c, a.astype(np.complex128) * b.astype(np.complex128)), TOL))
    w = oracle.window(oracle.WIN_BLACKMAN_HARRIS, 1024)
    y = np.full(n, np.nan, np.complex64)
    blk = pkg.clFFT(1024, pkg.CLFFT_FORWARD, w, pkg.DTYPE_COMPLEX, *GPU_ARGS, 1, 1, True)
    blk.work(8, [a], [y])
    checks.append(("clFFT 1024 x 8", relerr(y, oracle.fft_block(1024, True, w, True, oracle.DTYPE_COMPLEX, a, f64=True)), 2e-6))
    checks.append(("clFFT 1024 x 8: per-bin / per-frame bounds used", fft_used(blk, y, 1024, True, w, True, a), 1.0))
    taps = oracle.firdes_low_pass(1.0, 10e6, 1e6, 372000.0)
    xh = crandn(rng, n * 2 + taps.size - 1)
    yf = np.full(n, np.nan, np.complex64)
    pkg.clFilter(*GPU_ARGS, 2, taps, 1, 1).work(n, [xh], [yf])
    checks.append(("clFilter %d taps decim 2 x 8192" % taps.size, relerr(yf, conv64(xh, taps)[taps.size - 1::2][:n]), TOL))
    mag, ph = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    pkg.clComplexToMagPhase(*GPU_ARGS, 1).work(n, [a], [mag, ph])
    rm, rp = oracle.elem(5, n, [a])
    checks.append(("clComplexToMagPhase mag", relerr(mag, rm), TOL))
    checks.append(("clComplexToMagPhase phase", relerr(ph, rp), TOL))
    return checks


def _host_no_direct(pkg, oracle):
    checks = _host_small(pkg, oracle)
    ev = noted("MI355_NO_DIRECT")
    return result(ev is not None, ev, checks)


def _host_spin(pkg, oracle):
    return result(None, "", _host_small(pkg, oracle))


def _host_chunks(pkg, oracle):
    """1 MiB staging chunks, copied by the calling thread with plain memcpy: many pieces per call"""
    rng = np.random.default_rng(12)
    checks = []
    n = 700000
    a, b = crandn(rng, n), crandn(rng, n)
    c = np.full(n, np.nan, np.complex64)
    pkg.clMathOp(pkg.DTYPE_COMPLEX, *GPU_ARGS, pkg.MATHOP_MULTIPLY, 1).work(n, [a, b], [c])
    checks.append(("clMathOp multiply 700000", relerr(c, a.astype(np.complex128) * b.astype(np.complex128)), TOL))
    nt, d, nout = 129, 3, 400000
    taps = (rng.standard_normal(nt) / np.sqrt(nt)).astype(np.float32)
    xh = crandn(rng, nout * d + nt - 1)
    yf = np.full(nout, np.nan, np.complex64)
    pkg.clFilter(*GPU_ARGS, d, taps, 1, 1).work(nout, [xh], [yf])
    checks.append(("clFilter 129 taps decim 3 x 400000", relerr(yf, conv64(xh, taps)[nt - 1::d][:nout]), TOL))
    x = crandn(rng, 100 * 4096)
    y = np.full(x.size, np.nan, np.complex64)
    blk = pkg.clFFT(4096, pkg.CLFFT_FORWARD, [], pkg.DTYPE_COMPLEX, *GPU_ARGS, 1, 1, False)
    blk.work(100, [x], [y])
    checks.append(("clFFT 4096 x 100", relerr(y, oracle.fft_block(4096, True, None, False, oracle.DTYPE_COMPLEX, x, f64=True)), 2e-6))
    checks.append(("clFFT 4096 x 100: per-bin / per-frame bounds used", fft_used(blk, y, 4096, True, None, False, x), 1.0))
    ev = [noted(k) for k in ("MI355_CHUNK_MB", "MI355_COPY_STREAM", "MI355_COPY_THREADS")]
    return result(all(e is not None for e in ev), " | ".join(str(e) for e in ev), checks)


GROUPS["host_no_direct"] = {"MI355_NO_DIRECT": "1", "MI355_SPIN_US": "0"}
GROUPS["host_spin"] = {"MI355_SPIN_US": "0"}
GROUPS["host_chunks"] = {"MI355_CHUNK_MB": "1", "MI355_COPY_STREAM": "0", "MI355_COPY_THREADS": "0"}
add("host_no_direct", _host_no_direct, group="host_no_direct", switches=["MI355_NO_DIRECT"])
add("host_spin_us", _host_spin, group="host_spin", switches=["MI355_SPIN_US"], taken=None)
add("host_chunks", _host_chunks, group="host_chunks", switches=["MI355_CHUNK_MB", "MI355_COPY_STREAM", "MI355_COPY_THREADS"])


def _math_grid(pkg, oracle):
    import torch
    n = torch.cuda.get_device_properties(0).multi_processor_count * 256 * 4 * 40 + 5
    g = torch.Generator(device="cuda").manual_seed(3)
    a, b = (torch.randn(n * 2, device="cuda", generator=g) for _ in range(2))
    c = torch.full((n * 2,), float("nan"), device="cuda")
    pkg.clMathOp(pkg.DTYPE_COMPLEX, *GPU_ARGS, pkg.MATHOP_MULTIPLY_CONJUGATE, 1).work_device(n, [a, b], [c])
    torch.cuda.synchronize()
    za, zb = (t.cpu().numpy().view(np.complex64).astype(np.complex128) for t in (a, b))
    return result(None, "", [("clMathOp multiply conjugate x %d" % n, relerr(c.cpu().numpy().view(np.complex64), za * np.conj(zb)), TOL)])


add("math_wg_per_cu", _math_grid, {"MI355_MATH_WG_PER_CU": "1"}, taken=None)


# -------------------------------------------------------------------------------------------- clxcorrelate_fft_vcf: its pieces

def xcorr_route_kind(pkg, n):
    """the multiples (fft_ref.XCORR_MULT) a correlator of n points is held to: `direct` for the fused kernel (powers of two 16 ... 4096); for the
    composed route the kind of the clFFT route its transforms take -- a clFFT of that length, one frame, last_route().  Returns (kind, route)."""
    import torch
    from fft_ref import fft_bound_kind
    if 16 <= n <= 4096 and n & (n - 1) == 0:
        return "direct", "k_xcorr<%d>" % n
    blk = pkg.clFFT(n, pkg.CLFFT_FORWARD, [], pkg.DTYPE_COMPLEX, *GPU_ARGS, 0, 1, False)
    x = torch.zeros((n, 2), device="cuda")
    x[0, 0] = 1.0
    blk.work_device(1, [x], [torch.empty((n, 2), device="cuda")])
    torch.cuda.synchronize()
    route = blk.last_route()
    return fft_bound_kind(route), route


def xcorr_used(got, n, itype, ins, kind):
    """the largest used fraction of the per-lag and per-frame bounds of tests/fft_ref.py (bound 1.0) of ONE output against the float64
    definition of (reference, signal); a zero frame that did not come out as zeros counts as inf"""
    from fft_ref import xcorr_bound_check, xcorr_frames64
    (mag, sc), = xcorr_frames64(n, itype, ins)
    return max(xcorr_bound_check(got, mag, sc, n, itype, kind, check=False))


def _xcorr_device_pieces(pkg, oracle):
    """65536 points, two inputs, 2 x 256 + 3 frames through work_device: three pieces of the 128 MiB work buffers"""
    import torch
    from fft_ref import np_xcorr as _np_xcorr
    n, frames = 65536, 2 * 256 + 3
    ocl, sel, plat, dev = GPU_ARGS
    kind, route = xcorr_route_kind(pkg, n)
    blk = pkg.clxcorrelate_fft_vcf(n, 2, ocl, sel, plat, dev, 2)
    g = torch.Generator(device="cuda").manual_seed(21)
    ins = [torch.randn(frames * n * 2, device="cuda", generator=g) for _ in range(2)]
    out = torch.full((frames * n,), float("nan"), device="cuda")
    blk.work_device(frames, ins, [out])
    torch.cuda.synchronize()
    checks = []
    for f in six(frames):
        xs = [t[f * n * 2:(f + 1) * n * 2].cpu().numpy().view(np.complex64) for t in ins]
        got = out[f * n:(f + 1) * n].cpu().numpy()
        checks.append(("frame %d" % f, relerr(got, _np_xcorr(n, 2, xs)[0]), TOL))
        checks.append(("frame %d: per-lag / per-frame bounds used (%s)" % (f, kind), xcorr_used(got, n, 2, xs, kind), 1.0))
    return result(None, route, checks)


def _xcorr_host_pieces(pkg, oracle):
    """256 points, two inputs, 2 x 16384 + 5 frames through work(): three staging pieces of 64 MiB of input (16384 frames each); the first
    frame, the last one and the first of the second piece also bit for bit what work_device gives for that frame alone"""
    import torch
    from fft_ref import np_xcorr as _np_xcorr
    n, frames = 256, 2 * 16384 + 5
    rng = np.random.default_rng(22)
    ins = [rng.standard_normal(frames * n * 2, dtype=np.float32).view(np.complex64) for _ in range(2)]
    out = np.full(frames * n, np.nan, np.float32)
    ocl, sel, plat, dev = GPU_ARGS
    blk = pkg.clxcorrelate_fft_vcf(n, 2, ocl, sel, plat, dev, 2)
    blk.work(frames, ins, [out])
    checks = [("every frame", relerr(out, _np_xcorr(n, 2, ins)[0]), TOL),
              ("every frame: per-lag / per-frame bounds used", xcorr_used(out, n, 2, ins, "direct"), 1.0)]
    for f in (0, 16384, frames - 1):
        d_in = [torch.from_numpy(x[f * n:(f + 1) * n].view(np.float32).copy()).cuda() for x in ins]
        d_out = torch.full((n,), float("nan"), device="cuda")
        blk.work_device(1, d_in, [d_out])
        torch.cuda.synchronize()
        checks.append(("frame %d: work() against work_device, bits" % f, bits_differ(out[f * n:(f + 1) * n], d_out.cpu().numpy()), 0.0))
    return result(None, "", checks)


add("xcorr_fft_device_pieces", _xcorr_device_pieces, switches=[], taken=None)
add("xcorr_fft_host_pieces", _xcorr_host_pieces, switches=[], taken=None)


# --------------------------------------------------------------------------------------------------------------------- X-engine

_XE_DATA = {}  # geometry -> (input, [(window, first channel, last channel, reference)]): computed once, shared by the cases of a geometry


def xe_data(oracle, dtype, N, F, T, npol, nint, ends):
    """ends: the oracle's sums for the first, the middle and the last window of a launch of several; where one window alone costs the oracle more
    than a second, for the first, the middle and the last 64 channels of those (channels are independent, so the oracle runs on a 64-channel
    slice of the input).  Everything else of such a case is compared with the base route bit for bit"""
    key = (dtype, N, F, T, npol, nint, ends)
    if key not in _XE_DATA:
        if len(_XE_DATA) >= 3:
            _XE_DATA.clear()
        rng = np.random.default_rng(N * 1000 + T + npol + nint)
        if dtype == "cf32":
            x = crandn(rng, T * N * F * npol)
            refs = [(0, 0, F, oracle.xengine_cf32(N, F, npol, T, x))]
        else:
            x = rng.integers(-128, 128, size=(nint, T, N, F, npol * 2), dtype=np.int64).astype(np.int8)
            refs = []
            rows = N * npol
            sliced = ends and F > 192 and rows * (rows + 1) // 2 * F * T > 100e6  # (the oracle runs ~ 1e8 products a second)
            mid = (F // 2) // 64 * 64
            for i in (sorted({0, nint // 2, nint - 1}) if ends else range(nint)):
                for f0, f1 in (sorted({(0, 64), (mid, mid + 64), (F - 64, F)}) if sliced else [(0, F)]):
                    refs.append((i, f0, f1, oracle.xengine_ichar(N, f1 - f0, npol, T, np.ascontiguousarray(x[i, :, :, f0:f1]).reshape(-1), exact=True)))
        _XE_DATA[key] = (x, refs)
    return _XE_DATA[key]


def run_xe(pkg, oracle, dtype, N, F, T, npol, nint=1, ends=False):
    """(output, worst bit / relative error against the oracle, last_route()).  int8: device path (one call of nint windows); complex float:
    xcorrelate() on host buffers"""
    import torch
    x, refs = xe_data(oracle, dtype, N, F, T, npol, nint, ends)
    if dtype == "cf32":
        blk = pkg.clXEngine(*GPU_ARGS, True, pkg.DTYPE_COMPLEX, npol, N, pkg.CLXCORR_TRIANGULAR_ORDER, 0, F, T, [])
        out = np.full(blk.get_output_buffer_size(), np.nan, np.complex64)
        blk.xcorrelate(x, out)
        err = relerr(out, refs[0][3])
    else:
        blk = pkg.clXEngine(*GPU_ARGS, True, pkg.DTYPE_BYTE, npol, N, pkg.CLXCORR_TRIANGULAR_ORDER, 0, F, T, [])
        d_x = torch.from_numpy(x.reshape(-1)).cuda()
        per = blk.get_output_buffer_size()
        d_out = torch.full((nint * per * 2,), float("nan"), device="cuda")
        if nint == 1:
            blk.xcorrelate_device(d_x, d_out)
        else:
            blk.xcorrelate_n_device(nint, d_x, d_out)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(np.complex64)
        v = out.reshape(nint, F, -1)
        err = max(bits_differ(v[i, f0:f1].reshape(-1), r) for i, f0, f1, r in refs)
    route = blk.last_route()
    blk.stop()
    return out, err, route


def xe_case(name, env, geo, expect, dtype="i8", base=None, nint=1, switches=None, ends=False):
    """expect: 'differs' / 'equals' -- last_route() under env against last_route() under base (the default routing unless given); None: the
    route has no field for it.  int8: bit-exact against the oracle's integer sums and against the base run; complex float: <= 1e-5"""
    base = dict(base or {})

    def fn(pkg, oracle):
        N, F, T, npol = geo
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(base)
        o0, e0, r0 = run_xe(pkg, oracle, dtype, N, F, T, npol, nint, ends)
        os.environ.update(env)
        o1, e1, r1 = run_xe(pkg, oracle, dtype, N, F, T, npol, nint, ends)
        tag = "%s %d x %d x %d frames, %d pol, %d window(s)" % (dtype, N, F, T, npol, nint)
        if dtype == "cf32":
            checks = [(tag + " base route", e0, TOL), (tag, e1, TOL)]
        else:
            checks = [(tag + " base route against the integer sums", e0, 0.0), (tag + " against the integer sums", e1, 0.0),
                      (tag + " against the base route", bits_differ(o1, o0), 0.0)]
        tk = None if expect is None else ((r0 != r1) if expect == "differs" else (r0 == r1))
        return result(tk, "%s -> %s" % (r0, r1), checks)
    return add(name, fn, dict(base, **env), None, switches if switches is not None else list(env), None if expect is None else True)


_TWO = {"MI355_XE_NO_FUSED": "1"}
xe_case("xe_no_fused", _TWO, (64, 64, 256, 1), "differs")
xe_case("xe_no_fused_two_pol", _TWO, (33, 10, 130, 2), "equals")  # (rows of 40 bytes: never the fused kernel's)
xe_case("xe_no_lds", {"MI355_XE_NO_LDS": "1"}, (64, 64, 256, 1), "differs", base=_TWO)
xe_case("xe_slow_turn", {"MI355_XE_SLOW_TURN": "1"}, (128, 64, 256, 1), "differs")
xe_case("xe_slabs", {"MI355_XE_SLABS": "3"}, (128, 64, 256, 1), "differs", base={"MI355_XE_SLOW_TURN": "1"})
xe_case("xe_no_sb", {"MI355_XE_NO_SB": "1"}, (128, 64, 256, 1), "differs")
xe_case("xe_no_sb8", {"MI355_XE_NO_SB8": "1"}, (128, 64, 256, 1), "differs")
xe_case("xe_no_sb_corr", {"MI355_XE_NO_LDS": "1"}, (128, 64, 256, 1), "differs", base={"MI355_XE_NO_SB": "1"}, switches=["MI355_XE_NO_LDS", "MI355_XE_NO_SB"])
xe_case("xe_fused_whole_lines", {"MI355_XE_FUSED_WHOLE_LINES": "1"}, (20, 72, 96, 1), "differs")
xe_case("xe_fused_whole_kblocks", {"MI355_XE_FUSED_WHOLE_KBLOCKS": "1"}, (64, 64, 100, 1), "differs")
xe_case("xe_tsplit", {"MI355_XE_TSPLIT": "4", "MI355_XE_INKERNEL_REDUCE": "0"}, (64, 64, 256, 1), "differs")
xe_case("xe_inkernel_reduce", {"MI355_XE_INKERNEL_REDUCE": "1"}, (64, 64, 256, 1), "differs", base={"MI355_XE_TSPLIT": "4", "MI355_XE_INKERNEL_REDUCE": "0"},
        switches=["MI355_XE_INKERNEL_REDUCE"])
for _n, _e in (("no_compact", {"MI355_XE_NO_COMPACT": "1"}), ("no_pack24", {"MI355_XE_NO_PACK24": "1"}), ("no_pingpong", {"MI355_XE_NO_PINGPONG": "1"}),
               ("scale_f64", {"MI355_XE_SCALE_F64": "1"})):
    xe_case("xe_" + _n, _e, (64, 64, 256, 1), "equals")
    xe_case("xe_" + _n + "_two_pol", _e, (32, 64, 512, 2), "equals")
xe_case("xe_reduce_ipw", {"MI355_XE_REDUCE_IPW": "3"}, (64, 64, 256, 1), None)
xe_case("xe_wait_us", {"MI355_XE_WAIT_US": "5"}, (64, 64, 256, 1), None, base={"MI355_XE_TSPLIT": "4", "MI355_XE_INKERNEL_REDUCE": "1"})
xe_case("xe_no_prefetch", {"MI355_XE_NO_PREFETCH": "1"}, (64, 512, 256, 1), None, ends=True)
xe_case("xe_pf", {"MI355_XE_PF": "19"}, (64, 512, 256, 1), None, ends=True)
_BATCH = dict(geo=(64, 512, 32, 1), nint=10, base={"MI355_XE_NO_LINES": "1"}, ends=True)  # more units than CUs, several windows per launch
xe_case("xe_slow_first", {"MI355_XE_SLOW_FIRST": "1"}, (64, 512, 128, 1), None, nint=9, base={"MI355_XE_NO_LINES": "1"}, ends=True)  # (with the early touches on)
xe_case("xe_no_slow_first", {"MI355_XE_NO_SLOW_FIRST": "1"}, expect=None, **_BATCH)
xe_case("xe_no_persist", {"MI355_XE_NO_PERSIST": "1"}, (64, 512, 128, 1), None, nint=12, base={"MI355_XE_NO_LINES": "1"}, ends=True)
# the whole-line kernel: 8 windows of 1024 channels = 512 units, two per workgroup
_LINES = dict(geo=(64, 1024, 32, 1), nint=8, ends=True)
xe_case("xe_no_lines", {"MI355_XE_NO_LINES": "1"}, expect="differs", **_LINES)
xe_case("xe_lines_max_items", {"MI355_XE_LINES_MAX_ITEMS": "1"}, expect="differs", **_LINES)
xe_case("xe_lines_rot", {"MI355_XE_LINES_ROT": "0"}, expect="equals", **_LINES)
xe_case("xe_lines_pub", {"MI355_XE_LINES_PUB": "0"}, expect="equals", **_LINES)
xe_case("xe_lines_pf", {"MI355_XE_LINES_PF": "0"}, (64, 512, 160, 1), None, nint=8, ends=True)  # (five K blocks: longer than the touches' distance)
xe_case("xe_lines_pace", {"MI355_XE_LINES_PACE": "0"}, (64, 512, 160, 1), None, nint=8, ends=True)
xe_case("xe_lines_min_units", {"MI355_XE_LINES_MIN_UNITS": "4"}, (64, 128, 96, 1), "differs", nint=3)
xe_case("xe_lines_split_any", {"MI355_XE_LINES_SPLIT_ANY": "1", "MI355_XE_TSPLIT": "4"}, (64, 128, 256, 1), "differs", nint=2, switches=["MI355_XE_LINES_SPLIT_ANY", "MI355_XE_TSPLIT"])
xe_case("xe_no_lines_split", {"MI355_XE_NO_LINES_SPLIT": "1"}, (64, 1024, 512, 1), "differs", ends=True)  # (four ranges of four K blocks: one window of config 5, halved)
xe_case("xe_no_lines2", {"MI355_XE_NO_LINES2": "1"}, (64, 1024, 32, 2), "differs", ends=True)
xe_case("xe_no_split", {"MI355_XE_NO_SPLIT": "1"}, (64, 1024, 32, 1), "differs", nint=5, ends=True)
# complex float
xe_case("xe_cf32_two_kernels", {"MI355_XE_CF32_TWO_KERNELS": "1"}, (64, 64, 256, 1), "differs", dtype="cf32")
xe_case("xe_cf32_two_kernels_two_pol", {"MI355_XE_CF32_TWO_KERNELS": "1"}, (16, 16, 64, 2), "differs", dtype="cf32")
xe_case("xe_cf32_ch", {"MI355_XE_CF32_CH": "4"}, (64, 64, 256, 1), "differs", dtype="cf32")
xe_case("xe_cf32_tsplit", {"MI355_XE_CF32_TSPLIT": "1"}, (64, 64, 256, 1), "differs", dtype="cf32")
xe_case("xe_cf32_valu", {"MI355_XE_CF32_VALU": "1"}, (64, 64, 256, 1), "differs", dtype="cf32")
xe_case("xe_cf32_pad_copy", {"MI355_XE_CF32_PAD_COPY": "1"}, (20, 37, 128, 1), None, dtype="cf32")
xe_case("xe_cf32_no_pad", {"MI355_XE_CF32_NO_PAD": "1"}, (20, 37, 128, 1), "differs", dtype="cf32")


# -------------------------------------------------------------------------------- the evidence check itself: a switch that is not set

GROUPS["unset"] = {}
# the one-wave case in a process WITHOUT the variable: the transforms are right, and the evidence must say "not taken"
fft_case("fft_wave_geo_unset", [(256, 3 * 4096 // 256 + 1)], group="unset", note="MI355_FFT_WAVE_GEO", switches=[], taken=False, modes=["fwd"])


def group_cases(group):
    return [c for c in CHILD.values() if c.group == group]


def child_main(group):
    """run every case of a group in this (fresh) process; one JSON line per case on stdout"""
    root = os.path.dirname(HERE)
    sys.path.insert(0, root)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    oracle = entry.load_oracle()
    oracle.lib()
    install_log(pkg)
    for c in group_cases(group):
        saved = {k: os.environ.get(k) for k in c.env}
        os.environ.update(c.env)
        try:
            r = c.fn(pkg, oracle)
        except Exception as e:
            if device_error(e):  # the device may be in no state to go on -- nothing further is started, here or by the parent
                print("DEVICE ERROR in %s: %s" % (c.name, e), flush=True)
                sys.exit(FAULT_EXIT)
            raise
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        r["case"] = c.name
        print("CASE " + json.dumps(r), flush=True)
    print("GROUP DONE " + group, flush=True)


if __name__ == "__main__":
    child_main(sys.argv[1])
