"""GPU: clDedisperser against tests/dedisp_ref.py (numpy float32, the contract's summation order).  The order is pinned, so every
comparison is np.array_equal(..., equal_nan=True): there is no tolerance anywhere.  Inputs are seeded signed Gaussian float32 -- a sum
taken in another order differs in its last bits -- and every device call runs on guard-banded buffers (tests/guarded.py) whose output
interior is NaN before the call.

Routes, as csrc/dedisp.hip and the header state them:
  tiled    max - min <= 128 over the entries that are not -1 of every (16 trials, 8 channels) tile of the table: k_dd_tiled
  generic  every other table and every handle under set_generic(True): k_dd_gen
_tiled() below restates that rule; every test asserts the route it expects.

Geometries stay small (R <= 4, F <= 80, D <= 40, n <= 300, H <= 200); the one exception is the host path's n = 2000, the smallest
call that work() stages in more than one piece.

On an MI355X the file takes 3.9 s (56 tests).
"""
import ctypes as C
import functools
import glob
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import beamform_ref
import dedisp_ref as ref
import guarded

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
FB, DT, TT, SPREAD = 8, 16, 256, 128  # the tile sizes route() names (asserted in test_route_names_its_tiles) and the LDS plan's spread


def _tiled(tab):
    D, F = tab.shape
    for d0 in range(0, D, DT):
        for f0 in range(0, F, FB):
            v = tab[d0:d0 + DT, f0:f0 + FB]
            v = v[v >= 0]
            if v.size and int(v.max()) - int(v.min()) > SPREAD:
                return False
    return True


def _route_of(tab):
    return "tiled" if _tiled(tab) else "generic"


def _helper_table(D, F, H):
    """monotone, from the library's own helper: L-band, 1 ms, dispersion measures up to the one that fills H"""
    top_dm = H * 1e-3 / (ref.KDM * (1200.0 ** -2 - (1200.0 + 300.0 * (F - 1) / max(F, 1)) ** -2)) if F > 1 else 0.0
    tab, top = ref.delays(1200.0, 300.0 / F, F, 1e-3, np.linspace(0.0, 0.98 * top_dm, D))
    assert top <= H
    return tab


@functools.lru_cache(maxsize=None)
def _case(kind, R, F, D, H, n, seed=0):
    """(x, table), read-only"""
    rng = np.random.default_rng(7000 + seed + R * 3 + F * 5 + D * 7 + H * 11 + n * 13)
    x = ref.gaussian(rng, n + H, R, F)
    if kind == "helper":
        tab = _helper_table(D, F, H)
    elif kind == "helper2":  # the helper's table with a seeded wobble of 0 .. 2 samples
        tab = np.clip(_helper_table(D, F, H) + rng.integers(0, 3, size=(D, F)), 0, H).astype(np.int32)
    elif kind == "zeros":
        tab = np.zeros((D, F), np.int32)
    elif kind == "random":
        tab = ref.random_table(rng, D, F, H)
    elif kind == "smooth":
        tab = ref.smooth_table(rng, D, F, H)
    elif kind == "killed":  # channels, whole trials and single entries of -1
        tab = ref.smooth_table(rng, D, F, H)
        tab[:, F // 3] = -1
        tab[D // 2, :] = -1
        tab[rng.random((D, F)) < 0.1] = -1
        tab[D - 1, :] = -1
    else:
        raise ValueError(kind)
    x.setflags(write=False)
    tab.setflags(write=False)
    return x, tab


@functools.lru_cache(maxsize=None)
def _want(kind, R, F, D, H, n, seed=0):
    x, tab = _case(kind, R, F, D, H, n, seed)
    y = ref.dedisperse(x, tab, n, ref.TRIAL_MAJOR)  # [r][d][t]
    y.setflags(write=False)
    return y


def _run(blk, x, n, pitch=None, in_off=0, out_off=0, interior=True):
    """work_device on guard-banded buffers; returns [r][d][t] for either order (and checks that a pitched call left the gaps alone)"""
    import torch
    R, D = blk.num_rows, blk.num_trials
    xin = np.array(x, np.float32).reshape(-1)[:blk.in_floats(n)]  # (a writable copy: the cached cases are read-only)
    wi, vi = guarded.guarded_input(xin, guarded.pad_items(4, blk.in_floats_per_sample()), in_off, "cuda")
    n_out = blk.out_floats(n, pitch)
    wo, vo = guarded.guarded_output(n_out, np.float32, guarded.pad_items(4, blk.out_floats_per_sample()), out_off, "cuda")
    assert blk.work_device(n, [vi], [vo], pitch) == n
    torch.cuda.synchronize()
    guarded.check_guards(wi, vi, "input")
    gaps = blk.order == ref.TRIAL_MAJOR and pitch is not None and pitch > n
    guarded.check_guards(wo, vo, "output", interior=interior and not gaps)
    got = guarded.to_numpy(vo)
    if blk.order == ref.TIME_MAJOR:
        return np.ascontiguousarray(got.reshape(n, R, D).transpose(1, 2, 0))
    p = n if pitch is None else pitch
    full = np.full(R * D * p, np.nan, np.float32)  # (numpy's NaN is guarded.NAN_BITS: the last series' gap is not part of the buffer)
    full[:got.size] = got
    full = full.reshape(R * D, p)
    # the floats between n and out_pitch keep their prefill bit for bit
    assert np.all(np.ascontiguousarray(full[:, n:]).view(np.uint32) == guarded.NAN_BITS), "a gap float was written"
    return np.ascontiguousarray(full[:, :n]).reshape(R, D, n)


def _both_routes(blk, expect_route):
    """yields the route names after asserting them: the table's own route, then the forced generic one"""
    assert blk.route().startswith(expect_route), blk.route()
    yield blk.route()
    blk.set_generic(True)
    assert blk.route().startswith("generic"), blk.route()
    yield blk.route()
    blk.set_generic(False)
    assert blk.route().startswith(expect_route)


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# kind, R, F, D, H, n, route
FIXED = [
    ("helper", 2, 80, 40, 200, 300, "tiled"),   # monotone, from the library's helper; more than one tile along every axis
    ("helper", 1, 64, 33, 150, 257, "tiled"),
    ("zeros", 2, 33, 17, 5, 100, "tiled"),      # the plain channel sum
    ("random", 2, 40, 20, 200, 120, "generic"),  # non-monotone, spread up to 200: the LDS plan declines it
    ("random", 2, 40, 20, 120, 120, "tiled"),   # non-monotone, spread up to 120: it fits
    ("random", 1, 80, 40, 128, 300, "tiled"),   # the widest window the plan holds
    ("random", 1, 16, 16, 129, 64, "generic"),  # one sample wider
    ("smooth", 2, 20, 18, 0, 70, "tiled"),      # H = 0
    ("smooth", 2, 20, 18, 30, 1, "tiled"),      # n = 1
    ("smooth", 2, 1, 18, 30, 70, "tiled"),      # F = 1
    ("smooth", 2, 20, 1, 30, 70, "tiled"),      # D = 1
    ("smooth", 3, 20, 18, 30, 70, "tiled"),     # R = 3
    ("smooth", 1, 7, 15, 40, 255, "tiled"),     # F, D, n one below a tile
    ("smooth", 1, 9, 17, 40, 257, "tiled"),     # one above
    ("smooth", 2, 79, 33, 60, 255, "tiled"),
    ("smooth", 2, 24, 32, 60, 256, "tiled"),    # exact multiples
    ("killed", 3, 30, 20, 50, 90, "tiled"),     # channels, whole trials and entries of -1
    ("killed", 2, 30, 20, 200, 90, "generic"),  # the same on a table the plan declines
]


def test_route_names_its_tiles(gpu, pkg):
    blk = pkg.clDedisperser(*GPU_ARGS, 2, 20, 18, 30)
    assert blk.route() == "tiled R=2 F=20 D=18 fb=%d dt=%d tt=%d" % (FB, DT, TT)
    blk.set_generic(True)
    assert blk.route() == "generic R=2 F=20 D=18"
    assert (blk.in_floats_per_sample(), blk.history(), blk.out_floats_per_sample()) == ref.plan(2, 20, 18, 30)


@pytest.mark.parametrize("order", [ref.TIME_MAJOR, ref.TRIAL_MAJOR])
@pytest.mark.parametrize("kind,R,F,D,H,n,route", FIXED)
def test_fixed(gpu, pkg, kind, R, F, D, H, n, route, order):
    x, tab = _case(kind, R, F, D, H, n)
    assert _route_of(tab) == route
    want = _want(kind, R, F, D, H, n)
    if kind == "killed":
        assert not want[:, D - 1].any() and not np.signbit(want[:, D - 1]).any()  # a whole trial of -1 is +0.0
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
    for r in _both_routes(blk, route):
        got = _run(blk, x, n)
        assert _eq(got, want), (r, int(np.argmax(got != want)))
    blk.stop()


def test_trial_major_pitch(gpu, pkg):
    kind, R, F, D, H, n = "smooth", 3, 20, 18, 30, 70
    x, tab = _case(kind, R, F, D, H, n)
    want = _want(kind, R, F, D, H, n)
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TRIAL_MAJOR, tab)
    for r in _both_routes(blk, "tiled"):
        for pitch in (n, n + 5):
            assert _eq(_run(blk, x, n, pitch), want), (r, pitch)


@pytest.mark.parametrize("kind,H,route", [("smooth", 60, "tiled"), ("random", 200, "generic")])
def test_split_invariance(gpu, pkg, kind, H, route):
    """a stream taken as 1, 7, 64, 130, 98 outputs per call equals one call; TRIAL_MAJOR fills its long series through the pitch"""
    R, F, D, n = 2, 24, 20, 300
    x, tab = _case(kind, R, F, D, H, n)
    want = _want(kind, R, F, D, H, n)
    for order in (ref.TIME_MAJOR, ref.TRIAL_MAJOR):
        blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
        for r in _both_routes(blk, route):
            parts, t0 = [], 0
            for m in (1, 7, 64, 130, 98):
                parts.append(_run(blk, x[t0:t0 + m + H], m))
                t0 += m
            assert t0 == n and _eq(np.concatenate(parts, axis=2), want), (r, order)


def test_trial_major_series_filled_over_several_calls(gpu, pkg):
    """one output buffer with out_pitch = 300, written by three calls at time offsets 0, 100, 230"""
    import torch
    kind, R, F, D, H, n = "smooth", 2, 24, 20, 60, 300
    x, tab = _case(kind, R, F, D, H, n)
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TRIAL_MAJOR, tab)
    wi, vi = guarded.guarded_input(x.reshape(-1), guarded.pad_items(4, R * F), 0, "cuda")
    wo, vo = guarded.guarded_output(R * D * n, np.float32, guarded.pad_items(4, R * D), 0, "cuda")
    for r in _both_routes(blk, "tiled"):
        vo.fill_(float("nan"))
        for t0, m in ((0, 100), (100, 130), (230, 70)):
            blk.work_device(m, [vi[t0 * R * F:]], [vo[t0:]], n)
        torch.cuda.synchronize()
        guarded.check_guards(wi, vi, "input")
        guarded.check_guards(wo, vo, "output")
        assert _eq(guarded.to_numpy(vo).reshape(R, D, n), _want(kind, R, F, D, H, n)), r


@pytest.mark.parametrize("order", [ref.TIME_MAJOR, ref.TRIAL_MAJOR])
def test_alignment(gpu, pkg, order):
    """`in` and `out` 4, 8 and 12 bytes past a 16-byte boundary: the bits of the aligned call"""
    kind, R, F, D, H, n = "smooth", 3, 20, 18, 30, 70
    x, tab = _case(kind, R, F, D, H, n)
    want = _want(kind, R, F, D, H, n)
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
    for r in _both_routes(blk, "tiled"):
        for in_off, out_off in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1), (1, 2)):
            assert _eq(_run(blk, x, n, None, in_off, out_off), want), (r, in_off, out_off)


def test_nan_and_inf_reach(gpu, pkg):
    """one NaN, one +Inf, a NaN in a killed channel and a NaN in the last look-ahead sample: non-finite outputs exactly where the formula
    puts them"""
    R, F, D, H, n = 2, 20, 18, 30, 270
    x, tab = (a.copy() for a in _case("smooth", R, F, D, H, n))
    fk, fl = 5, 11
    tab[:, fk] = -1          # the killed channel
    tab[D - 1, fl] = H       # somebody uses the last look-ahead sample of channel fl
    ta, ra, fa = 40, 0, 3
    ti, ri, fi = 200, 1, 17
    x[ta, ra, fa] = np.nan
    x[ti, ri, fi] = np.inf
    x[:, :, fk] = np.nan
    x[n + H - 1, 1, fl] = np.nan
    expect = np.zeros((R, D, n), bool)
    for (t, r, f) in ((ta, ra, fa), (ti, ri, fi), (n + H - 1, 1, fl)):
        for d in range(D):
            if tab[d, f] >= 0 and 0 <= t - tab[d, f] < n:
                expect[r, d, t - tab[d, f]] = True
    assert expect[1, D - 1, n - 1] and expect[1, :, n - 1].sum() == (tab[:, fl] == H).sum()
    want = ref.dedisperse(x, tab, n, ref.TRIAL_MAJOR)
    assert np.array_equal(~np.isfinite(want), expect) and np.isnan(want[ra]).sum() > 0 and np.isposinf(want[ri]).sum() > 0
    for order in (ref.TIME_MAJOR, ref.TRIAL_MAJOR):
        blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
        for r in _both_routes(blk, "tiled"):
            got = _run(blk, x, n, interior=False)
            assert np.array_equal(~np.isfinite(got), expect), r
            assert _eq(got, want), r


@pytest.mark.parametrize("H,route", [(50, "tiled"), (200, "generic")])
def test_exact_integers(gpu, pkg, H, route):
    """inputs 0 .. 255, F = 80: every order is exact, so numpy int64 sums over fancy indices are an independent yardstick for the indexing"""
    R, F, D, n = 2, 80, 20, 150
    rng = np.random.default_rng(99 + H)
    xi = rng.integers(0, 256, size=(n + H, R, F))
    tab = ref.random_table(rng, D, F, H, kill=0.05)
    assert _route_of(tab) == route
    t = np.arange(n)
    want = np.zeros((R, D, n), np.int64)
    for d in range(D):
        keep = np.nonzero(tab[d] >= 0)[0]
        rows = t[:, None] + tab[d, keep][None, :]
        want[:, d, :] = xi[rows, :, keep[None, :]].sum(axis=1).T
    assert want.max() < 1 << 24
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TIME_MAJOR, tab)
    for r in _both_routes(blk, route):
        got = _run(blk, xi.astype(np.float32), n)
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), r


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    R, F, D, H = 2, 8, 4, 3
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TIME_MAJOR)
    tm = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TRIAL_MAJOR)
    L, h = pkg.lib(), blk._h
    buf = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    p = buf.data_ptr()
    vp = C.c_void_p
    # one output sample reads (1 + 3) 16 floats = 256 bytes and writes 8 floats = 32 bytes
    assert L.mi355_dedisp_work_dev(h, 1, vp(p + 2), vp(p + 4096), 0, None) == -1      # in not 4-byte aligned
    assert L.mi355_dedisp_work_dev(h, 1, vp(p), vp(p + 4096 + 2), 0, None) == -1      # out not 4-byte aligned
    assert L.mi355_dedisp_work_dev(h, 1, vp(p), vp(p + 252), 0, None) == -1           # out starts inside the look-ahead
    assert L.mi355_dedisp_work_dev(h, 1, vp(p + 28), vp(p), 0, None) == -1            # in starts inside out
    assert L.mi355_dedisp_work_dev(h, 1, vp(p), vp(p + 4096), 1, None) == -1          # TIME_MAJOR takes out_pitch 0 only
    assert L.mi355_dedisp_work_dev(tm._h, 5, vp(p), vp(p + 4096), 4, None) == -1      # out_pitch < n
    assert L.mi355_dedisp_work_dev(tm._h, 1, vp(p + 200), vp(p), 9, None) == -1       # the pitched extent counts: 7 x 9 + 1 floats reach into in
    assert L.mi355_dedisp_work_dev(h, 1, None, vp(p), 0, None) == -1
    assert L.mi355_dedisp_work_dev(h, 1, vp(p), None, 0, None) == -1
    assert L.mi355_dedisp_work_dev(h, -1, vp(p), vp(p + 4096), 0, None) == -1
    assert L.mi355_dedisp_work_dev(h, (1 << 40) // 64, vp(p), vp(p + 4096), 0, None) == -3            # n + H samples of 64 bytes pass 2^40
    assert L.mi355_dedisp_work_dev(tm._h, 2, vp(p), vp(p + 4096), (1 << 40) // 32 + 1, None) == -3    # 8 series of that pitch pass 2^40
    assert L.mi355_dedisp_work(h, 1, vp(p + 2), vp(p + 4096), 0) == -1
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0  # nothing was launched


def test_zero_outputs_is_a_no_op(gpu, pkg):
    import torch
    blk = pkg.clDedisperser(*GPU_ARGS, 2, 8, 4, 3)
    out = torch.full((256,), 7.0, dtype=torch.float32, device="cuda")
    assert pkg.lib().mi355_dedisp_work_dev(blk._h, 0, None, C.c_void_p(out.data_ptr()), 0, None) == 0
    assert pkg.lib().mi355_dedisp_work(blk._h, 0, None, None, 0) == 0
    assert blk.work_device(0, [out], [out]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_set_delays_round_trip_and_route(gpu, pkg):
    R, F, D, H, n = 2, 80, 40, 200, 120
    x, smooth = _case("helper", R, F, D, H, n)
    _, wild = _case("random", R, F, D, H, n)
    assert _route_of(smooth) == "tiled" and _route_of(wild) == "generic"
    blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H)
    assert not blk.delays().any() and blk.route().startswith("tiled")  # no table: all zero
    blk.set_delays(smooth)
    assert np.array_equal(blk.delays(), smooth) and blk.route().startswith("tiled")
    assert _eq(_run(blk, x, n), ref.dedisperse(x, smooth, n, ref.TRIAL_MAJOR))
    blk.set_delays(wild)  # a legal update that changes the route, and route() says so
    assert np.array_equal(blk.delays(), wild) and blk.route().startswith("generic")
    assert _eq(_run(blk, x, n), _want("random", R, F, D, H, n))
    for v in (-2, H + 1):
        bad = smooth.copy()
        bad[3, 7] = v
        with pytest.raises(pkg.Mi355Error):
            blk.set_delays(bad)
        assert np.array_equal(blk.delays(), wild) and blk.route().startswith("generic")  # a refused update changes nothing
    assert _eq(_run(blk, x, n), _want("random", R, F, D, H, n))
    blk.set_delays(smooth)
    assert blk.route().startswith("tiled")
    with pytest.raises(ValueError):
        blk.set_delays(smooth[:-1])


def test_set_delays_between_enqueued_calls(gpu, pkg):
    """two work_dev calls on one stream with set_delays between them and no synchronisation: the old table entirely, then the new one"""
    import torch
    R, F, D, H, n = 2, 80, 40, 200, 120
    x, smooth = _case("helper", R, F, D, H, n)
    _, wild = _case("random", R, F, D, H, n)
    _, smooth2 = _case("helper2", R, F, D, H, n)
    assert _route_of(smooth) == _route_of(smooth2) == "tiled" and _route_of(wild) == "generic" and not np.array_equal(smooth, smooth2)
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    for order in (ref.TIME_MAJOR, ref.TRIAL_MAJOR):
        blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, smooth)
        for first, second in ((smooth, smooth2), (smooth2, wild), (wild, smooth)):
            blk.set_delays(first)
            o1 = torch.full((n * R * D,), float("nan"), dtype=torch.float32, device="cuda")
            o2 = torch.full_like(o1, float("nan"))
            torch.cuda.synchronize()
            blk.work_device(n, [d_x], [o1])
            blk.set_delays(second)
            blk.work_device(n, [d_x], [o2])
            torch.cuda.synchronize()
            assert np.array_equal(o1.cpu().numpy(), ref.dedisperse(x, first, n, order).reshape(-1), equal_nan=True)
            assert np.array_equal(o2.cpu().numpy(), ref.dedisperse(x, second, n, order).reshape(-1), equal_nan=True)


def test_host_work_equals_device_work(gpu, pkg):
    kind, R, F, D, H, n = "smooth", 3, 20, 18, 30, 70
    x, tab = _case(kind, R, F, D, H, n)
    want = _want(kind, R, F, D, H, n)
    tm = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TIME_MAJOR, tab)
    y = np.full(n * R * D, np.nan, np.float32)
    assert tm.work(n, [x], [y]) == n
    assert _eq(y.reshape(n, R, D).transpose(1, 2, 0), want) and _eq(_run(tm, x, n), want)
    tr = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, ref.TRIAL_MAJOR, tab)
    pitch = n + 5
    z = np.full(R * D * pitch, np.nan, np.float32)
    assert tr.work(n, [x], [z], pitch) == n
    z = z.reshape(R * D, pitch)
    assert _eq(z[:, :n].reshape(R, D, n), want) and np.isnan(z[:, n:]).all()
    with pytest.raises(ValueError):
        tm.work(n + 1, [x], [y])


def test_host_work_in_pieces(gpu, pkg):
    """n = 2000 outputs of 4 x 80 floats: 2.5 MB, which work() stages in three pieces of whole samples with their look-ahead"""
    R, F, D, H, n = 4, 80, 40, 100, 2000
    x, tab = _case("smooth", R, F, D, H, n)
    want = _want("smooth", R, F, D, H, n)
    for order in (ref.TIME_MAJOR, ref.TRIAL_MAJOR):
        blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
        y = np.full(n * R * D, np.nan, np.float32)
        assert blk.work(n, [x], [y]) == n
        got = y.reshape(n, R, D).transpose(1, 2, 0) if order == ref.TIME_MAJOR else y.reshape(R, D, n)
        assert _eq(got, want), order


def _sweep_geometries(count=40, seed=2026):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        R, F, D = int(rng.integers(1, 5)), int(rng.integers(1, 81)), int(rng.integers(1, 41))
        n, H = int(rng.integers(1, 301)), int(rng.integers(0, 201))
        kind = ("random", "smooth", "killed")[int(rng.integers(0, 3))]
        out.append((kind, R, F, D, H, n, int(rng.integers(0, 2)), int(rng.integers(1 << 20))))
    return out


def test_random_sweep(gpu, pkg):
    """40 seeded geometries and tables within the file's bounds: the reference's bits on both routes, either order"""
    routes = {"tiled": 0, "generic": 0}
    for kind, R, F, D, H, n, order, seed in _sweep_geometries():
        x, tab = _case(kind, R, F, D, H, n, seed)
        want = ref.dedisperse(x, tab, n, ref.TRIAL_MAJOR)
        expect = _route_of(tab)
        routes[expect] += 1
        blk = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
        got = [_run(blk, x, n) for _ in _both_routes(blk, expect)]
        geo = (kind, R, F, D, H, n, order)
        assert _eq(got[0], want), geo
        assert _eq(got[1], want) and _eq(got[0], got[1]), geo
        blk.stop()
    assert routes["tiled"] >= 5 and routes["generic"] >= 5, routes  # both routes occur among the geometries' own choices


def test_beamformer_feeds_the_dedisperser(gpu, pkg):
    """int8 frames -> clBeamformer POWER (stokes_i) -> clDedisperser, all on the device, equal to beamform_ref followed by dedisp_ref;
    a dispersed pulse in the frames peaks on its own trial"""
    import torch
    S, B, F, npol, Ti, D, n = 4, 2, 24, 2, 2, 12, 60
    tab, H = ref.delays(1500.0, -300.0 / F, F, 1e-3, np.arange(D) * 3.0)
    assert 20 < H <= 200 and _tiled(tab)
    rng = np.random.default_rng(77)
    T = n + H
    frames = rng.integers(-3, 4, size=(T * Ti, S, F, npol, 2), dtype=np.int8)
    k, tp = 8, 21
    for f in range(F):
        w0 = tp + tab[k, f]
        frames[w0 * Ti:(w0 + 1) * Ti, :, f, :, 0] = 60  # the pulse, dispersed as trial k
    w = np.zeros((F, npol, B, S, 2), np.int8)
    w[:, :, 0, :, 0] = 1                                 # beam 0: the plain sum of the stations
    w[:, :, 1] = rng.integers(-20, 21, size=(F, npol, S, 2), dtype=np.int8)
    power = beamform_ref.power(frames, w, Ti, True)      # [T][B][F] float32: the dedisperser's x[t][r][f]
    want = ref.dedisperse(power, tab, n, ref.TRIAL_MAJOR)
    assert np.unravel_index(np.argmax(want[0]), want[0].shape) == (k, tp)
    bf = pkg.clBeamformer(*GPU_ARGS, beamform_ref.POWER, npol, S, F, B, Ti, True, w)
    dd = pkg.clDedisperser(*GPU_ARGS, B, F, D, H, ref.TRIAL_MAJOR, tab)
    assert bf.out_items_per_unit() == dd.in_floats_per_sample()
    d_frames = torch.from_numpy(frames.reshape(-1)).cuda()
    wm, vm = guarded.guarded_output(T * B * F, np.float32, guarded.pad_items(4, B * F), 0, "cuda")
    wo, vo = guarded.guarded_output(B * D * n, np.float32, guarded.pad_items(4, B * D), 0, "cuda")
    for r in _both_routes(dd, "tiled"):
        vm.fill_(float("nan"))
        vo.fill_(float("nan"))
        assert bf.work_device(T, [d_frames], [vm]) == T
        assert dd.work_device(n, [vm], [vo]) == n
        torch.cuda.synchronize()
        guarded.check_guards(wm, vm, "filterbank")
        guarded.check_guards(wo, vo, "output")
        assert np.array_equal(guarded.to_numpy(vm), power.reshape(-1))
        got = guarded.to_numpy(vo).reshape(B, D, n)
        assert _eq(got, want), r
        assert np.unravel_index(np.argmax(got[0]), got[0].shape) == (k, tp)


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, n + history() - 1 samples in, n items of R D floats out"""
    mod = _pybind()
    kind, R, F, D, H, n = "smooth", 3, 20, 18, 30, 70
    x, tab = _case(kind, R, F, D, H, n)
    want = _want(kind, R, F, D, H, n).transpose(2, 0, 1).reshape(-1)
    dd = mod.clDedisperser(*GPU_ARGS, R, F, D, H, tab.reshape(-1))
    assert dd.history() == H + 1 and dd.max_delay() == H and dd.route().startswith("tiled")
    assert np.array_equal(dd.delays(), tab.reshape(-1))
    y = np.full(n * R * D, np.nan, np.float32)
    assert dd.work(n, [x.reshape(-1)], [y]) == n
    assert np.array_equal(y, want)
    dd.set_generic(True)
    assert dd.route().startswith("generic")
    y[:] = np.nan
    assert dd.work(n, [x.reshape(-1)], [y]) == n and np.array_equal(y, want)
    z = mod.clDedisperser(*GPU_ARGS, R, F, D, H)
    assert not z.delays().any()
    z.set_delays(tab.reshape(-1))
    y[:] = np.nan
    assert z.work(n, [x.reshape(-1)], [y]) == n and np.array_equal(y, want)
    with pytest.raises(ValueError):
        z.set_delays(tab.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        z.work(n + 1, [x.reshape(-1)], [y])  # one sample more than offered
    with pytest.raises(ValueError):
        mod.clDedisperser(*GPU_ARGS, R, F, D, -1)


def test_cli_row(gpu):
    """test-clenabled-mi355 --dedisp-only prints the checksum of a small run on generated samples"""
    r = subprocess.run([CLI, "--dedisp-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    R, F, D, T = 2, 20, 5, 70
    H = (D - 1) * (F - 1) // 4
    state, vals = 12345, np.empty((T + H) * R * F, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    x = (vals - 256 * (vals > 127)).astype(np.float32).reshape(T + H, R, F)
    tab = np.array([[d * (F - 1 - f) // 4 for f in range(F)] for d in range(D)], np.int32)
    tab[2, 3] = -1
    y = ref.dedisperse(x, tab, T, ref.TIME_MAJOR).reshape(-1).astype(np.int64)
    want = int(((np.arange(y.size) % 7 + 1) * y).sum())
    assert re.search(r"^clDedisperser checksum (-?\d+)$", r.stdout, re.M).group(1) == str(want), r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clDedisperser (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout
