"""GPU: clAccelResampler against tests/accel_ref.py.

The block moves 32-bit words, so every comparison is np.array_equal on uint32 views, on both routes (route() is asserted), with every
device buffer guard-banded (tests/guarded.py), NaN words in the gaps of a pitched input and an output whose interior holds NaN words
before the call: a word of a pitch gap that the call wrote shows as well as one it skipped.

Shapes: N = 256 (one short tile), 4099 (odd: a last tile of three outputs, every head and tail path) and 8192 (eight tiles) with the
table {0, +1, -1, +2^63/N, -2^63/N, two random values, apex}, which fits one group of eight trials; N = 16384, where the same unsorted
table is spread too widely for two trials to share a window (group = 1) and its sorted form takes a group in between; and N = 2^22 at the
two extreme coefficients, whose windows lie half a million samples from their tiles."""
import functools
import glob
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import accel_ref as ref
import dedisp_ref
import guarded
import psearch_ref
import ssearch_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
ROUTES = pytest.mark.parametrize("generic", [False, True], ids=["tiled", "generic"])


@functools.lru_cache(maxsize=None)
def _table(N, sort=False):
    rng = np.random.default_rng(N + 1)
    top = ref.cmax(N)
    t = [0, 1, -1, top, -top] + [int(v) for v in rng.integers(-top, top, 2, dtype=np.int64)] + [ref.apex(N)]
    return tuple(sorted(t)) if sort else tuple(t)


@functools.lru_cache(maxsize=None)
def _x(S, N):
    w = ref.words(np.random.default_rng(S + N), S, N)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _want(S, N, table):
    out = ref.resample(_x(S, N), table)
    out.setflags(write=False)
    return out


def _block(pkg, S, N, table, generic):
    blk = pkg.clAccelResampler(*GPU_ARGS, S, N, np.array(table, np.int64))
    blk.set_generic(generic)
    _route(blk, S, N, table, generic)
    return blk


def _route(blk, S, N, table, generic):
    want = "generic S=%d N=%d A=%d" % (S, N, len(table)) if generic else \
        "tiled S=%d N=%d A=%d tile=%d group=%d" % (S, N, len(table), ref.TILE, ref.group(N, list(table)))
    assert blk.route() == want, blk.route()


def _buffers(x, rows, ip, op, in_off, out_off):
    S, N = x.shape
    wi, vi = guarded.guarded_input(ref.pitched(x, ip).view(np.int32), guarded.pad_items(4, N), in_off, "cuda")
    wo, vo = guarded.guarded_output((rows - 1) * op + N, np.int32, guarded.pad_items(4, N), out_off, "cuda")
    return wi, vi, wo, vo


def _rows(wi, vi, wo, vo, rows, N, op):
    """the guards, the gaps of the output (still NaN words) and the rows as uint32 [rows][N]"""
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "output", interior=False)
    got = guarded.to_numpy(vo).view(np.uint32)
    gap = np.ones(got.size, bool)
    for r in range(rows):
        gap[r * op:r * op + N] = False
    assert (got[gap] == guarded.NAN_BITS).all(), "a word between n and out_pitch was written"
    return ref.unpitched(got, rows, N, op)


def _run(blk, x, a0=0, na=None, ip=None, op=None, in_off=0, out_off=0):
    """work_device on guard-banded buffers; x uint32 [S][N] -> uint32 [S][na][N]"""
    import torch
    S, N = x.shape
    na = blk.num_trials - a0 if na is None else na
    ip, op = N if ip is None else ip, N if op is None else op
    wi, vi, wo, vo = _buffers(x, S * na, ip, op, in_off, out_off)
    assert blk.work_device([vi], [vo], a0, na, ip, op) == 1
    torch.cuda.synchronize()
    return _rows(wi, vi, wo, vo, S * na, N, op).reshape(S, na, N)


def _same(got, want):
    assert got.dtype == np.uint32 and want.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    return True


def _apex_inside(N, table, S, op, off):
    """series whose apex row has the apex run strictly inside one of the tiled route's lane runs, `out` off words past a 16-byte
    boundary"""
    first, last = ref.apex_run(N, table[-1])
    assert last - first + 1 < 8
    hit = []
    for s in range(S):
        word = off + (s * len(table) + len(table) - 1) * op
        hit += [s for f, l in ref.lane_runs(N, word) if f < first and last < l]
    return hit


@ROUTES
@pytest.mark.parametrize("N", [256, 4099, 8192])
def test_small_shapes_equal_the_reference(gpu, pkg, N, generic):
    """S = 3, the eight-trial table in one group; dense, and at in_pitch = N + 6, out_pitch = N + 10 with `in` and `out` 4, 8 and 12
    bytes past a 16-byte boundary.  The apex trial moves only the samples next to N / 2 by one more than their neighbours: for one of
    the offsets that run lies strictly inside a lane's run of four (asserted), where a shift taken from the run's ends would miss it"""
    S, table = 3, _table(N)
    first, last = ref.apex_run(N, table[-1])
    assert ref.delta(N, table[-1], first) == 2 and ref.delta(N, table[-1], first - 1) == 1 and last - first + 1 < 8
    blk = _block(pkg, S, N, table, generic)
    want = _want(S, N, table)
    assert _same(_run(blk, _x(S, N)), want)
    inside = 0
    for off in (1, 2, 3):
        assert _same(_run(blk, _x(S, N), ip=N + 6, op=N + 10, in_off=off, out_off=off), want)
        assert _same(_run(blk, _x(S, N), ip=N + 6, op=N + 10, in_off=(off + 1) % 4, out_off=off), want)
        inside += len(_apex_inside(N, table, S, N + 10, off))
    assert inside > 0, "the apex run never lay strictly inside a lane's run"


@ROUTES
@pytest.mark.parametrize("sort", [False, True], ids=["unsorted", "sorted"])
def test_spread_table_shrinks_the_group(gpu, pkg, sort, generic):
    """N = 16384: +2^63/N next to -2^63/N differ by 4096 samples at mid-series, more than a window holds, so the plan takes one trial
    per group; sorted, neighbours lie closer and the group is larger but below the table's eight"""
    S, N = 2, 16384
    table = _table(N, sort)
    g = ref.group(N, list(table))
    assert g == 1 if not sort else 1 < g < 8, g
    blk = _block(pkg, S, N, table, generic)
    assert _same(_run(blk, _x(S, N), ip=N + 6, op=N + 10, in_off=1, out_off=3), _want(S, N, table))


@ROUTES
def test_large_shape(gpu, pkg, generic):
    """S = 1, N = 2^22, c = +-2^63 / N: shifts of up to 524288 samples, windows far from their tiles, 32 MiB of output"""
    S, N = 1, 1 << 22
    table = (ref.cmax(N), -ref.cmax(N))
    want = _want(S, N, table)
    shift = ref.src_array(N, table[0]) - np.arange(N)
    assert shift.max() == 524288
    blk = _block(pkg, S, N, table, generic)
    assert _same(_run(blk, _x(S, N), op=N + 10, in_off=1, out_off=2), want)


@ROUTES
def test_splits_equal_the_single_call(gpu, pkg, generic):
    """trial ranges [0, 3) + [3, A), one trial at a time, and the series split over two handles"""
    S, N = 3, 4099
    table = _table(N)
    A = len(table)
    want = _want(S, N, table)
    blk = _block(pkg, S, N, table, generic)
    kw = dict(ip=N + 6, op=N + 10, in_off=3, out_off=1)
    assert _same(np.concatenate([_run(blk, _x(S, N), 0, 3, **kw), _run(blk, _x(S, N), 3, A - 3, **kw)], axis=1), want)
    assert _same(np.concatenate([_run(blk, _x(S, N), a, 1, **kw) for a in range(A)], axis=1), want)
    parts = [_run(_block(pkg, ns, N, table, generic), _x(S, N)[s0:s0 + ns], **kw) for s0, ns in ((0, 1), (1, 2))]
    assert _same(np.concatenate(parts, axis=0), want)
    assert blk.series_to_trial(0) == (0, 0) and blk.series_to_trial(2 * A + 3) == (2, 3) and blk.series_to_trial(4, 3, 2) == (2, 3)
    with pytest.raises(ValueError):
        blk.series_to_trial(S * A)


@ROUTES
def test_set_trials_between_two_enqueued_calls(gpu, pkg, generic):
    """two calls enqueued behind one another with a set_trials between them, nothing waited for: each uses its own table entirely
    (and the tiled route its own group size: the second table is the spread one)"""
    import torch
    S, N = 3, 16384
    first, second = _table(N, True), _table(N, False)
    blk = _block(pkg, S, N, first, generic)
    A = len(first)
    x = _x(S, N)
    b1, b2 = _buffers(x, S * A, N, N, 0, 0), _buffers(x, S * A, N + 6, N + 10, 1, 1)
    assert blk.work_device([b1[1]], [b1[3]]) == 1
    blk.set_trials(np.array(second, np.int64))
    assert blk.work_device([b2[1]], [b2[3]], 0, A, N + 6, N + 10) == 1
    torch.cuda.synchronize()
    _route(blk, S, N, second, generic)
    assert np.array_equal(blk.trials(), np.array(second, np.int64))
    assert _same(_rows(*b1, S * A, N, N).reshape(S, A, N), _want(S, N, first))
    assert _same(_rows(*b2, S * A, N, N + 10).reshape(S, A, N), _want(S, N, second))
    with pytest.raises(ValueError):
        blk.set_trials(np.zeros(A - 1, np.int64))
    with pytest.raises(pkg.Mi355Error):
        blk.set_trials(np.array([ref.cmax(N) + 1] * A, np.int64))
    assert np.array_equal(blk.trials(), np.array(second, np.int64))  # a refused update keeps the table


@ROUTES
def test_host_work_equals_work_device(gpu, pkg, generic):
    S, N = 3, 4099
    table = _table(N)
    blk = _block(pkg, S, N, table, generic)
    want = _want(S, N, table)
    assert _same(_run(blk, _x(S, N)), want)
    assert _same(blk.resample(_x(S, N)), want)
    A = len(table)
    buf = ref.pitched(_x(S, N), N + 6)
    out = np.full((S * 5 - 1) * (N + 10) + N, guarded.NAN_BITS, np.uint32)
    assert blk.work([buf], [out], 2, 5, N + 6, N + 10) == 1
    assert _same(ref.unpitched(out, S * 5, N, N + 10).reshape(S, 5, N), want[:, 2:7])
    gap = np.ones(out.size, bool)
    for r in range(S * 5):
        gap[r * (N + 10):r * (N + 10) + N] = False
    assert (out[gap] == guarded.NAN_BITS).all()
    # float32 buffers are taken as they are
    y = np.empty((S, A, N), np.float32)
    assert blk.work([_x(S, N).view(np.float32)], [y]) == 1 and _same(y.view(np.uint32), want)


def test_host_work_in_pieces_and_trial_runs(gpu, pkg):
    """S = 3 series of 2^19 words are two staged pieces (2 + 1 series), ten trials two runs (8 + 2) per piece; the ladder comes from
    accel_trials"""
    S, N, tsamp = 3, 1 << 19, 64e-6
    da = 8 * ref.LIGHT / (tsamp * N * N)
    table, count = pkg.accel_trials(N, tsamp, -4.5 * da, 5.5 * da, 1.0)
    assert count == 10 and 0 in table.tolist()
    table = tuple(int(v) for v in table)
    blk = _block(pkg, S, N, table, False)
    assert _same(blk.resample(_x(S, N)), _want(S, N, table))


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    S, N, A = 3, 256, 4
    blk = _block(pkg, S, N, (0, 1, -1, 5), False)
    x = torch.zeros(S * N + 16, dtype=torch.int32, device="cuda")
    wy, y = guarded.guarded_output(S * A * N + 16, np.int32, guarded.pad_items(4, 64), 0, "cuda")
    L, vp = pkg.lib(), lambda t, off=0: t.data_ptr() + off
    #        in     in_pitch  out   out_pitch a0 na
    bad = [(None, N, vp(y), N, 0, A), (vp(x), N, None, N, 0, A), (vp(x, 2), N, vp(y), N, 0, A), (vp(x), N, vp(y, 1), N, 0, A),
           (vp(x), N - 1, vp(y), N, 0, A), (vp(x), N, vp(y), N - 1, 0, A), (vp(x), N, vp(y), N, -1, 2), (vp(x), N, vp(y), N, 0, 0),
           (vp(x), N, vp(y), N, 0, A + 1), (vp(x), N, vp(y), N, 3, 2), (vp(x), N, vp(y), N, A, 1), (vp(x), N, vp(y), N, 2 ** 31 - 1, 2),
           (vp(x), N, vp(x, 4 * (S * N - 1)), N, 0, 1),                         # the last input word is the first output word
           (vp(y, 4 * (S * N - 1)), N, vp(y), N, 0, 1), (vp(x), N, vp(x), N, 0, A),
           (vp(x), (1 << 38) // S + 1, vp(y), N, 0, A), (vp(x), N, vp(y), (1 << 38) // (S * A) + 1, 0, A)]
    for a in bad:
        rc = L.mi355_accel_work_dev(blk._h, *a, None)
        assert rc == (-3 if max(a[1], a[3]) > 1 << 30 else -1), (a, L.mi355_last_error().decode())
    hx, hy = np.zeros(S * N, np.uint32), np.full(S * A * N, guarded.NAN_BITS, np.uint32)
    for ip, op, a0, na in ((N - 1, N, 0, A), (N, N - 1, 0, A), (N, N, 1, A), (N, N, 0, 0)):   # the same checks on the host path
        assert L.mi355_accel_work(blk._h, hx.ctypes.data, ip, hy.ctypes.data, op, a0, na) == -1
    assert L.mi355_accel_work(blk._h, hx.ctypes.data, N, hx.ctypes.data, N, 0, 1) == -1 and (hy == guarded.NAN_BITS).all()
    torch.cuda.synchronize()
    guarded.check_guards(wy, y, "output of a refused call", interior=False)
    assert (y == guarded.NAN_BITS).all(), "a refused call wrote"
    with pytest.raises(ValueError):
        blk.work_device([x[:S * N - 1]], [y])
    with pytest.raises(ValueError):
        blk.work_device([x], [y[:S * A * N - 1]])
    with pytest.raises(pkg.Mi355Error):
        pkg.clAccelResampler(*GPU_ARGS, S, N, [ref.cmax(N) + 1])


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu, pkg):
    """the C++ block as the scheduler calls it: work() on numpy buffers, two segments in, two items of S A rows out, equal to the
    yardstick bit for bit"""
    mod = _pybind()
    S, N = 3, 4099
    table = _table(N)
    A = len(table)
    want = _want(S, N, table)
    ar = mod.clAccelResampler(*GPU_ARGS, S, N, np.array(table, np.int64))
    assert ar.history() == 1 and ar.segment_len() == N and ar.num_trials() == A and ar.rows() == S * A
    assert np.array_equal(ar.trials(), np.array(table, np.int64))
    x = _x(S, N).view(np.float32)
    two = np.concatenate([x.reshape(-1), x.reshape(-1)])
    for generic in (False, True):
        ar.set_generic(generic)
        assert ar.route().startswith("generic " if generic else "tiled ")
        y = np.zeros((2, S, A, N), np.float32)
        assert ar.work(2, [two], [y]) == 2
        for item in range(2):
            assert _same(y[item].view(np.uint32), want)
    ar.set_trials(np.array(table[::-1], np.int64))
    y = np.zeros((1, S, A, N), np.float32)
    assert ar.work(1, [x.reshape(-1)], [y]) == 1 and _same(y[0].view(np.uint32), want[:, ::-1])
    with pytest.raises(ValueError):
        ar.set_trials(np.zeros(A - 1, np.int64))
    with pytest.raises(ValueError):
        ar.work(1, [x.reshape(-1)[:-1]], [y])
    with pytest.raises(ValueError):
        mod.clAccelResampler(*GPU_ARGS, S, 100, np.zeros(2, np.int64))


def test_cli_row(gpu):
    """test-clenabled-mi355 --accel-only resamples generated words at (S, n, A) = (2, 4099, 3), prints the checksum of its output,
    sum_j (j % 7 + 1) word_j modulo 2^64, and exits 0: the yardstick gives the same sum"""
    r = subprocess.run([CLI, "--accel-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    S, N = 2, 4099
    state, vals = 12345, np.empty(S * N, np.uint32)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state
    table = (0, ref.cmax(N), -ref.apex(N))
    out = ref.resample(vals.reshape(S, N), table).reshape(-1).astype(np.uint64)
    want = int(((np.arange(out.size, dtype=np.uint64) % np.uint64(7) + np.uint64(1)) * out).sum(dtype=np.uint64))
    assert "clAccelResampler checksum %d\n" % want in r.stdout, r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clAccelResampler (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout


def test_dedisperser_feeds_the_resampler_and_the_resampler_the_search(gpu, pkg):
    """clDedisperser -> clAccelResampler -> clPulseSearch.measure() -> clSpectralSearch, all on the device.  F = 64 channels, D = 2
    trials, N = 2^14: the dedispersed series of trial 1 is a train of pulses every 12.8 samples seen through the map of -c,
    c = (2^63 / N) / 16 (a drift of 128 samples at mid-observation), in unit noise; the trials are {-2c, -c, 0, c, 2c}.  First on the
    yardsticks alone, then on the device's records: the best record over all rows lies in (series 1, trial c), its fundamental within
    one bin of 1280, its S/N at least four times the best of trial 0 (the condition; about 18 in the yardstick)"""
    import torch
    F, D, N, d_true, period, H, Bb = 64, 2, 1 << 14, 1, 12.8, 5, 16
    c = ref.cmax(N) // 16
    trials = (-2 * c, -c, 0, c, 2 * c)
    A = len(trials)
    delay = np.rint(np.arange(D)[:, None] * 12.0 * (F - 1 - np.arange(F))[None, :] / (F - 1)).astype(np.int32)
    Hd = int(delay.max())
    rng = np.random.default_rng(11)
    x = rng.normal(1.0, 0.125, (N + Hd, 1, F)).astype(np.float32)   # the sum over the band: sigma 1
    y = np.zeros(N + Hd, np.float32)
    y[:N] = ref.pulse_train(N, period, -c)
    for f in range(F):
        x[delay[d_true, f]:, 0, f] += np.float32(2.0 / F) * y[:N + Hd - delay[d_true, f]]

    def verdict(pk, what):
        """pk: PEAK records [D * A][blocks]"""
        s, h, k = ssearch_ref.best(pk, Bb)
        top = pk["snr"].max(axis=1).reshape(D, A)
        print("%s: best row %d (series %d, trial %d), h = %d, k = %d, S/N %.1f; trial 0 at most %.1f" % (
            what, s, s // A, s % A, h, k, top.max(), top[:, 2].max()))
        assert (s // A, s % A) == (d_true, 3)
        assert abs(k / 2.0 ** h - N / period) <= 1.0
        assert top[d_true, 3] >= 4.0 * top[:, 2].max()

    series = dedisp_ref.dedisperse(x, delay, N, dedisp_ref.TRIAL_MAJOR).reshape(D, N)
    rows = ref.resample(series, trials).reshape(D * A, N)
    isg = psearch_ref.measure(rows.view(np.float32), N)[1].astype(np.float32)
    verdict(ssearch_ref.peaks(ssearch_ref.spectrum64(rows.view(np.float32), isg, 2).astype(np.float32), H, Bb), "yardsticks")

    dd = pkg.clDedisperser(*GPU_ARGS, 1, F, D, Hd, pkg.DEDISP_TRIAL_MAJOR, delay)
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    w_series, d_series = guarded.guarded_output(D * N, np.float32, guarded.pad_items(4, N), 0, "cuda")
    assert dd.work_device(N, [d_x], [d_series]) == N
    ss = None
    for generic in (False, True):
        ar = _block(pkg, D, N, trials, generic)
        w_rows, d_rows = guarded.guarded_output(D * A * N, np.float32, guarded.pad_items(4, N), 0, "cuda")
        assert ar.work_device([d_series], [d_rows]) == 1
        mean, d_isg = pkg.clPulseSearch(*GPU_ARGS, 1, D * A, 1, 16, pkg.PSEARCH_TRIAL_MAJOR).measure(d_rows, N)
        torch.cuda.synchronize()
        guarded.check_guards(w_series, d_series, "series")
        guarded.check_guards(w_rows, d_rows, "rows")
        assert np.array_equal(d_series.cpu().numpy().view(np.uint32), series.reshape(-1).view(np.uint32))
        assert _same(d_rows.cpu().numpy().view(np.uint32).reshape(D * A, N), rows)
        assert np.allclose(d_isg, isg, rtol=1e-6)
        ss = ss or pkg.clSpectralSearch(*GPU_ARGS, D * A, N, H, Bb, 2, pkg.SSEARCH_SERIES, d_isg)
        w_pk, d_pk = guarded.guarded_output(2 * D * A * ss.records, np.float32, guarded.pad_items(4, 2 * ss.records), 0, "cuda")
        assert ss.work_device([d_rows], [d_pk]) == 1
        torch.cuda.synchronize()
        guarded.check_guards(w_pk, d_pk, "peaks", interior=False)
        verdict(ss.peaks_of(d_pk).reshape(D * A, ss.records), "device, %s" % ar.route())
