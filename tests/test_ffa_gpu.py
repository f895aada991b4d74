"""GPU: clPeriodSearch against tests/ffa_ref.py (numpy float32, the contract's recursion stage by stage, the circular boxcars and the
64-bit key order).  The arithmetic is pinned, so every comparison is np.array_equal on raw bits: the 8-byte records, and the profiles
wherever the reference is not NaN; where it is NaN the device must be NaN too (positions compared as positions).  Every device call
runs on guard-banded buffers (tests/guarded.py) with NaN in the gaps of a pitched input; both outputs hold NaN bit patterns before the
call, and the floats j >= p of every profile row must still hold them afterwards.

Routes, as csrc/ffa.hip and the header state them:
  fused    every shape: k_ffa_pass, the stages in passes of q stages, q the largest with 2^q p_hi <= 32768 floats and at most 8, L
           split as evenly as that allows; 256 threads where a unit has at most 4096 pairs (and p_hi <= 2048), else 1024
  generic  every handle under set_generic(True): k_ffa_stage per stage, then k_ffa_eval
Every test asserts the route it expects through route().  The shapes are the issue's five plus one per pass plan they do not reach:
three passes (a middle pass that neither reads the input nor evaluates), two passes at 256 threads, and a shape whose base periods
do not fit one launch (the scratch plane holds two of its three base periods).

On an MI355X the file takes 6.5 s (115 tests)."""
import functools
import glob
import importlib.util
from fractions import Fraction
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import dedisp_ref
import ffa_ref as ref
import fold_ref
import guarded

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")

# (S, p_lo, p_hi, L, K) -> the fused route's pass plan and threads
SHAPES = {
    (1, 16, 16, 1, 1): "q=1 t=256",          # the smallest of everything
    (3, 16, 19, 3, 4): "q=3 t=256",          # several base periods, K at its limit for p_lo
    (2, 37, 40, 5, 5): "q=5 t=256",          # odd and prime rows
    (1, 4093, 4096, 4, 6): "q=2,2 t=1024",   # the longest rows, 256 KiB per series
    (2, 250, 251, 12, 7): "q=6,6 t=1024",    # the deepest tree, 4 MiB per series
    (1, 4095, 4096, 7, 2): "q=3,2,2 t=1024",  # three passes
    (1, 16, 17, 10, 2): "q=5,5 t=256",       # two passes at 256 threads
    (3, 250, 252, 12, 1): "q=6,6 t=1024",    # 3 x 4096 x 252 floats per base period: two base periods per launch, then one
}
SMALL = [s for s in SHAPES if s[0] * (s[2] << s[3]) <= 1 << 16]
KINDS = ["gamma", "stats", "pitch", "offset", "special", "noprofiles"]


def _stats(S):
    s = np.arange(S, dtype=np.float32)
    return (np.float32(6) + np.float32(0.25) * s).astype(np.float32), (np.float32(0.3) * (1 + np.float32(0.125) * s)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(shape, special=False):
    """x[S][N] float32, read-only"""
    S, p_lo, p_hi, L, K = shape
    N = p_hi << L
    rng = np.random.default_rng(7000 + S + 3 * p_lo + 5 * L + 7 * K)
    x = rng.gamma(2.0, 3.0, (S, N)).astype(np.float32)
    if special:
        m = 1 << L
        x[0, 3:3 + min(p_lo + 2, 40)] = -0.0            # a run of -0 from row 0 into row 1
        x[S - 1, (m // 2) * p_lo + 5] = np.nan          # (s, r, j) = (S - 1, m / 2, 5) of base period p_lo
        x[0, (m - 1) * p_lo + p_lo - 1] = np.inf        # the last bin of the last row of p_lo
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(shape, special=False, stats=False):
    S, p_lo, p_hi, L, K = shape
    m, g = _stats(S) if stats else (None, None)
    peaks, prof = ref.search(_case(shape, special), S, p_lo, p_hi, L, K, m, g, profiles=_want(shape, special, False)[1] if stats else None)
    peaks.setflags(write=False)
    prof.setflags(write=False)
    return peaks, prof


def _block(pkg, shape, stats=False):
    m, g = _stats(shape[0]) if stats else (None, None)
    return pkg.clPeriodSearch(*GPU_ARGS, *shape, m, g)


def _expect_route(blk, shape, generic=False):
    S, p_lo, p_hi, L, K = shape
    head = "%s S=%d p=%d..%d L=%d K=%d" % ("generic" if generic else "fused", S, p_lo, p_hi, L, K)
    assert blk.route() == (head if generic else head + " " + SHAPES[shape]), blk.route()


def _run(blk, x, pitch=None, in_off=0, peaks_off=0, prof_off=0, profiles=True, sync=True):
    """work_device on guard-banded buffers; x[S][N].  Returns a function that checks the guards and gives (peaks [S][P][m], profiles
    [S][P][m][p_hi] or None)"""
    import torch
    S, N, P, m, p_hi = blk.num_series, blk.N, blk.num_periods, blk.num_rows, blk.p_hi
    row = N if pitch is None else pitch
    buf = np.full((S - 1) * row + N, np.nan, np.float32)
    for s in range(S):
        buf[s * row:s * row + N] = x[s]
    wi, vi = guarded.guarded_input(buf, guarded.pad_items(4, N), in_off, "cuda")
    wo, vo = guarded.guarded_output(2 * S * P * m, np.float32, guarded.pad_items(4, 2 * m), peaks_off, "cuda")
    outs = [vo]
    if profiles:
        wp, vp = guarded.guarded_output(S * P * m * p_hi, np.float32, guarded.pad_items(4, m * p_hi), prof_off, "cuda")
        outs.append(vp)
    assert blk.work_device([vi], outs, pitch) == 1

    def finish():
        torch.cuda.synchronize()
        guarded.check_guards(wi, vi, "input")
        guarded.check_guards(wo, vo, "peaks", interior=False)
        pk = blk.peaks_of(vo).reshape(S, P, m)
        if not profiles:
            return pk, None
        guarded.check_guards(wp, vp, "profiles", interior=False)
        return pk, guarded.to_numpy(vp).reshape(S, P, m, p_hi)
    return finish() if sync else finish


def _same(got, want, p_lo):
    """records bit for bit; profiles bit for bit where the reference is not NaN, NaN where it is; the prefill where j >= p"""
    pk, prof = got
    wpk, wprof = want
    assert np.array_equal(pk.view(np.uint64), wpk.view(np.uint64)), np.argwhere(pk.view(np.uint64) != wpk.view(np.uint64))[:4]
    if prof is None:
        return True
    gb, wb = prof.view(np.uint32), wprof.view(np.uint32)
    for pi in range(wprof.shape[1]):
        p = p_lo + pi
        assert (gb[:, pi, :, p:] == guarded.NAN_BITS).all(), "a float j >= p of a profile row was written"
        nan = np.isnan(wprof[:, pi, :, :p])
        assert np.array_equal(np.isnan(prof[:, pi, :, :p]), nan), "NaN positions"
        assert np.array_equal(gb[:, pi, :, :p][~nan], wb[:, pi, :, :p][~nan]), (pi, np.argwhere((gb != wb)[:, pi, :, :p] & ~nan)[:4])
    return True


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "S%d_p%d-%d_L%d_K%d" % s)
def test_equals_the_reference(gpu, pkg, shape, kind, generic):
    stats, special = kind == "stats", kind == "special"
    blk = _block(pkg, shape, stats)
    blk.set_generic(generic)
    _expect_route(blk, shape, generic)
    if stats:
        m, g = blk.stats()
        assert np.array_equal(m, _stats(shape[0])[0]) and np.array_equal(g, _stats(shape[0])[1])
    x = _case(shape, special)
    want = _want(shape, special, stats)
    if special:
        assert np.isnan(want[1][..., :shape[1]]).any() and np.isinf(want[0]["snr"]).any()
    got = _run(blk, x, pitch=blk.N + 37 if kind == "pitch" else None, in_off=1 if kind == "offset" else 0,
               prof_off=3 if kind == "offset" else 0, peaks_off=2 if kind == "offset" else 0, profiles=kind != "noprofiles")
    assert _same(got, want, shape[1])


def test_nan_reach_is_what_the_formula_gives(gpu, pkg):
    """one NaN at x[s = 1][r p + j0] for p = 38: the NaN bins of every base period's profiles are those of the reference, series 0 has
    none, and records of profiles that are NaN throughout are {-Inf, 0xFFFFFFFF}"""
    shape = (2, 37, 40, 5, 5)
    x = np.array(_case(shape))
    x[1, 9 * 38 + 17] = np.nan
    want = ref.search(x, *shape)
    assert not np.isnan(want[1][0, :, :, :37]).any() and np.isnan(want[1][1, 1, :, :38]).sum() == 32
    for generic in (False, True):
        blk = _block(pkg, shape)
        blk.set_generic(generic)
        assert _same(_run(blk, x), want, shape[1])
    y = np.full((2, 16), np.nan, np.float32)
    blk = _block(pkg, (1, 16, 16, 1, 1))
    for generic in (False, True):
        blk.set_generic(generic)
        pk, prof = _run(blk, y.reshape(1, 32))
        assert (pk["loc"] == 0xFFFFFFFF).all() and np.isneginf(pk["snr"]).all() and np.isnan(prof).all()


@pytest.mark.parametrize("shape", SMALL + [(1, 4095, 4096, 7, 2)], ids=lambda s: "S%d_p%d-%d_L%d_K%d" % s)
def test_set_generic_back_and_forth(gpu, pkg, shape):
    blk = _block(pkg, shape, True)
    x, want = _case(shape), _want(shape, False, True)
    for generic in (False, True, False):
        blk.set_generic(generic)
        _expect_route(blk, shape, generic)
        assert _same(_run(blk, x), want, shape[1])


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_set_stats_between_two_enqueued_calls(gpu, pkg, generic):
    """the first call uses the old version entirely, the second the new one"""
    shape = (3, 16, 19, 3, 4)
    blk = _block(pkg, shape, False)
    blk.set_generic(generic)
    x = _case(shape)
    first = _run(blk, x, sync=False)
    blk.set_stats(*_stats(3))
    second = _run(blk, x, sync=False)
    assert _same(second(), _want(shape, False, True), 16) and _same(first(), _want(shape, False, False), 16)
    assert np.array_equal(blk.stats()[0], _stats(3)[0])
    with pytest.raises(ValueError):
        blk.set_stats(np.zeros(2, np.float32), np.zeros(2, np.float32))


@pytest.mark.parametrize("shape", [(3, 16, 19, 3, 4), (2, 37, 40, 5, 5)], ids=lambda s: "S%d_p%d-%d_L%d_K%d" % s)
def test_host_work_equals_the_reference(gpu, pkg, shape):
    """work() on numpy buffers, pitched, with and without profiles; search() and best()"""
    blk = _block(pkg, shape, True)
    x, want = _case(shape), _want(shape, False, True)
    S, N = shape[0], blk.N
    buf = np.full((S - 1) * (N + 5) + N, np.nan, np.float32)
    for s in range(S):
        buf[s * (N + 5):s * (N + 5) + N] = x[s]
    for generic in (False, True):
        blk.set_generic(generic)
        pk, prof = blk.search(buf, N + 5, profiles=True)
        assert _same((pk, prof), want, shape[1])
        assert np.array_equal(blk.search(x).view(np.uint64), want[0].view(np.uint64))
    s, pi, i = ref.best(want[0])
    bs, period, k, j, snr = blk.best(want[0])
    loc = int(want[0]["loc"][s, pi, i])
    assert (bs, period, k, j) == (s, shape[1] + pi + Fraction(int(i), blk.num_rows - 1), loc >> 24, loc & 0xFFFFFF)
    assert snr == float(want[0]["snr"][s, pi, i])


@pytest.mark.parametrize("profiles", [False, True], ids=["records", "profiles"])
def test_host_work_in_pieces(gpu, pkg, profiles):
    """a series of 4096 x 252 floats is more than the 4 MiB a staged piece of the host path holds, so the three series go one by one:
    every piece takes its own statistics, records and profiles"""
    shape = (3, 250, 252, 12, 1)
    blk = _block(pkg, shape, True)
    want = _want(shape, False, True)
    for generic in (False, True):
        blk.set_generic(generic)
        got = blk.search(_case(shape), profiles=profiles)
        assert _same(got if profiles else (got, None), want, shape[1])


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    blk = _block(pkg, (3, 16, 19, 3, 4))
    N, rec, prof = blk.N, 3 * blk.records, 3 * blk.profile_floats
    x = torch.zeros(3 * N + 8, dtype=torch.float32, device="cuda")
    y = torch.full((2 * rec + 8,), 7.0, dtype=torch.float32, device="cuda")
    z = torch.full((prof + 8,), 7.0, dtype=torch.float32, device="cuda")
    L, h, vp = pkg.lib(), blk._h, lambda t, off=0: t.data_ptr() + off
    for args in [(None, N, vp(y), vp(z)), (vp(x), N, None, vp(z)), (vp(x, 2), N, vp(y), vp(z)), (vp(x), N, vp(y, 4), vp(z)),
                 (vp(x), N, vp(y), vp(z, 2)), (vp(x), N - 1, vp(y), vp(z)), (vp(x), N, vp(x), vp(z)), (vp(x), N, vp(y), vp(x, 8)),
                 (vp(x), N, vp(y), vp(y, 16)), (vp(x), (1 << 38) // 3 + 1, vp(y), None)]:
        rc = L.mi355_ffa_work_dev(h, args[0], args[1], args[2], args[3], None)
        assert rc == (-3 if args[1] > 1 << 30 else -1), (args, L.mi355_last_error().decode())
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (z == 7.0).all()
    with pytest.raises(ValueError):
        blk.work_device([x[:3 * N - 1]], [y, z])


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_injected_pulsar_is_found(gpu, pkg, generic):
    """the recorded case of tests/test_ffa.py: the best record of all lies at (p, i) = (37, 11) with k = 2"""
    x = ref.pulsar(np.random.default_rng(7), 32 * 38, 37 + 11 / 31, 4, 3.0)
    blk = pkg.clPeriodSearch(*GPU_ARGS, 1, 36, 38, 5, 4, np.array([10], np.float32), np.array([0.5], np.float32))
    blk.set_generic(generic)
    want = ref.search(x, 1, 36, 38, 5, 4, [10.0], [0.5])
    got = _run(blk, x.reshape(1, -1))
    assert _same(got, want, 36)
    s, period, k, j, snr = blk.best(got[0])
    assert (s, period, k) == (0, 37 + Fraction(11, 31), 2) and snr > 12


def test_dedisperser_feeds_the_search_and_the_search_the_folder(gpu, pkg):
    """F = 64 channels, D = 4 trials, L = 5: a filterbank with a dispersed pulse of period 37 + 11/31 samples -> clDedisperser (per-trial
    output) -> clPeriodSearch, on the device: both equal to their references bit for bit, the best record lies at the injected trial
    and (p, i) = (37, 11); mi355_fold_model of mi355_ffa_period then drives clFolder on the same filterbank, bit-equal to fold_ref"""
    import torch
    F, D, L, K, d_true, tsamp = 64, 4, 5, 4, 2, 1e-3
    p_lo, p_hi, m = 36, 38, 32
    N = m * p_hi
    delay = np.rint(np.arange(D)[:, None] * 12.0 * (F - 1 - np.arange(F))[None, :] / (F - 1)).astype(np.int32)
    H = int(delay.max())
    rng = np.random.default_rng(11)
    x = rng.normal(1.0, 0.25, (N + H, 1, F)).astype(np.float32)   # the sum over the band: mean 64, sigma 2
    t = np.arange(N + H)
    for f in range(F):
        x[:, 0, f] += np.float32(3.0 / F) * (((t - delay[d_true, f] + 0.5) % (37 + 11 / 31)) < 4)
    series = dedisp_ref.dedisperse(x, delay, N, dedisp_ref.TRIAL_MAJOR).reshape(D, N)
    mean, isg = np.full(D, 64, np.float32), np.full(D, 0.5, np.float32)
    want = ref.search(series, D, p_lo, p_hi, L, K, mean, isg)
    s, pi, i = ref.best(want[0])
    assert (s, p_lo + pi, i) == (d_true, 37, 11)
    dd = pkg.clDedisperser(*GPU_ARGS, 1, F, D, H, pkg.DEDISP_TRIAL_MAJOR, delay)
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    d_series = torch.full((D * N,), float("nan"), dtype=torch.float32, device="cuda")
    assert dd.work_device(N, [d_x], [d_series]) == N
    blk = pkg.clPeriodSearch(*GPU_ARGS, D, p_lo, p_hi, L, K, mean, isg)
    for generic in (False, True):
        blk.set_generic(generic)
        d_pk = torch.full((2 * D * blk.records,), float("nan"), dtype=torch.float32, device="cuda")
        assert blk.work_device([d_series], [d_pk]) == 1
        torch.cuda.synchronize()
        assert np.array_equal(d_series.cpu().numpy().view(np.uint32), series.reshape(-1).view(np.uint32))
        pk = blk.peaks_of(d_pk).reshape(D, 3, m)
        assert np.array_equal(pk.view(np.uint64), want[0].view(np.uint64))
        bs, period, k, j, snr = blk.best(pk)
        assert (bs, period) == (d_true, 37 + Fraction(11, 31))
    nbin, Ts = 16, 64
    model = pkg.fold_model(pkg.ffa_period(37, L, 11, tsamp), 0.0, tsamp, 0.0).reshape(1, 3)
    fo = pkg.clFolder(*GPU_ARGS, 1, F, nbin, Ts, model)
    ns = N // Ts
    d_out = torch.full((ns * nbin * F,), float("nan"), dtype=torch.float32, device="cuda")
    assert fo.work_device(ns, [d_x], [d_out]) == ns
    torch.cuda.synchronize()
    out, _ = fold_ref.fold(x[:ns * Ts], model, 0, nbin, Ts)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), out.reshape(-1).view(np.uint32))


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, two segments in, two items of records and profiles out"""
    mod = _pybind()
    shape = (3, 16, 19, 3, 4)
    x, want = _case(shape), _want(shape, False, True)
    fs = mod.clPeriodSearch(*GPU_ARGS, *shape, *_stats(3))
    assert fs.history() == 1 and fs.segment_len() == 8 * 19 and fs.records_per_series() == 32 and fs.period(16, 7, 2.0) == 34.0
    assert np.array_equal(fs.mean(), _stats(3)[0]) and np.array_equal(fs.inv_sigma(), _stats(3)[1])
    two = np.concatenate([x.reshape(-1), x.reshape(-1)])
    for generic in (False, True):
        fs.set_generic(generic)
        assert fs.route().startswith("generic " if generic else "fused ")
        pk = np.zeros((2,) + want[0].shape, ref.PEAK)
        prof = np.full((2,) + want[1].shape, np.nan, np.float32)
        assert fs.work(2, [two], [pk, prof]) == 2
        for item in range(2):
            assert _same((pk[item], prof[item]), want, 16)
        pk[:] = 0
        assert fs.work(1, [x], [pk[:1]]) == 1 and np.array_equal(pk[0].view(np.uint64), want[0].view(np.uint64))
    with pytest.raises(ValueError):
        fs.set_stats(np.zeros(2, np.float32), np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        fs.work(1, [x.reshape(-1)[:-1]], [pk])  # one float fewer than the call reads
    with pytest.raises(ValueError):
        mod.clPeriodSearch(*GPU_ARGS, 3, 16, 19, 3, 6)


def test_cli_row(gpu):
    """test-clenabled-mi355 --ffa-only runs the smallest shape on generated samples, prints its checksum and exits 0"""
    r = subprocess.run([CLI, "--ffa-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    state, vals = 12345, np.empty(32, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    x = (vals + 1).astype(np.float32)
    peaks, prof = ref.search(x, 1, 16, 16, 1, 1)
    u = np.uint64

    def wsum(a, mod):
        a = a.reshape(-1).astype(u)
        return int(((np.arange(a.size, dtype=u) % u(mod) + u(1)) * a).sum(dtype=u))

    want = (wsum(peaks["snr"].view(np.uint32), 7) + wsum(peaks["loc"], 7) + wsum(prof.view(np.uint32), 5)) % (1 << 64)
    assert re.search(r"^clPeriodSearch checksum (\d+)$", r.stdout, re.M).group(1) == str(want), r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clPeriodSearch (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout
