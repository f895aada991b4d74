"""GPU: clFolder against tests/fold_ref.py (Python integers for the phase, numpy float32 additions in ascending time).  The phase is integer
and the summation order is pinned, so every comparison is np.array_equal on the raw bits of `out` and on `hits`.  Every device call runs
on guard-banded buffers (tests/guarded.py); `out` and `hits` hold NaN bit patterns before the call, so an item the call never wrote
shows.

Routes, as csrc/fold.hip and the header state them:
  bins     F a multiple of 64, every nbin and Ts: k_fold_index (per-bin lists) + k_fold_bins (a wave per (subint, row, channel group,
           run of bins); 4, 2 or 1 floats per lane by F % 256, F % 128)
  generic  every other shape and every handle under set_generic(True): k_fold_gen / k_fold_gen_hits
Every test asserts the route it expects through route().

Shapes stay small: the largest input is (2, 128, 5, 16384) with one sub-integration, 16 MiB."""
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
import fbclean_ref
import fold_ref as ref
import guarded

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
M64 = (1 << 64) - 1

# (R, F, nbin, Ts, sub-integrations)
BINS = [(1, 64, 2, 16, 3),        # the smallest of everything; one float per lane
        (2, 256, 16, 64, 2),      # four floats per lane
        (3, 320, 7, 48, 2),       # five groups of 64, nbin no power of two, Ts no power of two (the sort pads to 64)
        (1, 64, 4096, 16, 2),     # most bins empty
        (2, 128, 5, 16384, 1)]    # the longest sub-integration; two floats per lane
GENERIC = [(3, 52, 7, 48, 2), (1, 1, 3, 16, 3)]
KINDS = ["plain", "nu0", "fast", "nudot+", "nudot-", "t40", "wrap", "flags", "nan", "negzero"]


def _route_of(F):
    return "bins" if F % 64 == 0 else "generic"


def _models(kind, R, nbin, Ts):
    """[R][3] uint64: another model for every row"""
    m = np.empty((R, 3), np.uint64)
    for r in range(R):
        phi0 = (0x9E3779B97F4A7C15 * (r + 1)) & M64
        nu = (1 << 64) // (nbin + 3 + r) + 0x1234567 * (r + 1)      # a period of a little more than nbin samples
        nudot = 0
        if kind == "nu0":
            nu = 0
        elif kind == "fast":
            nu = (1 << 63) + (1 << 64) // (5 + r)                  # a period below two samples: aliases, but is defined
        elif kind in ("nudot+", "nudot-"):
            # over one sub-integration nudot Ts^2 / 2 moves the phase by more than a bin: the boundaries move inside it
            nudot = ((3 << 64) // (nbin * Ts * Ts) + 1 + r) * (1 if kind == "nudot+" else -1)
        elif kind in ("t40", "wrap"):
            nudot = -(1 << 20) - r if kind == "t40" else (1 << 3) + 1
        m[r] = ref.words(phi0, nu, nudot)
    return m


def _T0(kind, n):
    if kind == "t40":
        return (1 << 40) - 5
    if kind == "wrap":
        return (1 << 64) - n + 21          # T wraps to 0 inside the call
    return 12345 if kind in ("nudot+", "nudot-") else 0


@functools.lru_cache(maxsize=None)
def _case(kind, R, F, nbin, Ts, ns):
    """(x[n][R][F] float32, models[R][3] uint64, T0, tflags[n][R] uint8 or None), read-only"""
    rng = np.random.default_rng(9000 + R * 3 + F * 5 + nbin * 7 + Ts * 11 + ns + len(kind))
    n = ns * Ts
    x = rng.gamma(4.0, 0.25, (n, R, F)).astype(np.float32)
    models = _models(kind, R, nbin, Ts)
    tf = None
    if kind == "flags":
        # whole turns of row 0 and scattered samples of the last row
        tf = np.zeros((n, R), np.uint8)
        b = ref.bins(models[0], 0, n, nbin)
        turn = np.cumsum(np.r_[0, np.diff(b) < 0])
        tf[(turn == 1) | (turn == 2), 0] = 1
        tf[rng.random(n) < 0.2, R - 1] = 255
        tf.setflags(write=False)
    elif kind == "nan":
        x[n // 3, R // 2, F // 2] = np.nan
        x[n - 1, 0, F - 1] = np.inf
    elif kind == "negzero":
        x[:, R - 1, F // 3] = -0.0
    x.setflags(write=False)
    models.setflags(write=False)
    return x, models, _T0(kind, n), tf


@functools.lru_cache(maxsize=None)
def _want(kind, R, F, nbin, Ts, ns):
    x, models, T0, tf = _case(kind, R, F, nbin, Ts, ns)
    res = ref.fold(x, models, T0, nbin, Ts, tf)
    for a in res:
        a.setflags(write=False)
    return res


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def _same(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _run(blk, x, tf=None, in_off=0, out_off=0, hits=True, finite=True):
    """work_device on guard-banded buffers; x[n][R][F].  Returns (out, hits or None)"""
    import torch
    n, R, F = x.shape
    ns, nbin = n // blk.subint_len, blk.nbin
    wi, vi = guarded.guarded_input(x, guarded.pad_items(4, R * F), in_off, "cuda")
    wo, vo = guarded.guarded_output(ns * R * nbin * F, np.float32, guarded.pad_items(4, R * F), out_off, "cuda")
    wt = vt = wh = vh = None
    if tf is not None:
        wt, vt = guarded.guarded_input(tf.view(np.int8), guarded.pad_items(1, R), 0, "cuda")
    if hits:
        wh, vh = guarded.guarded_output(ns * R * nbin, np.int32, guarded.pad_items(4, R * nbin), 0, "cuda")
    assert blk.work_device(ns, [vi, vt], [vo, vh]) == ns
    torch.cuda.synchronize()
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "out", interior=finite)
    if tf is not None:
        guarded.check_guards(wt, vt, "tflags")
    got = [guarded.to_numpy(vo).reshape(ns, R, nbin, F), None]
    if hits:
        guarded.check_guards(wh, vh, "hits")
        got[1] = guarded.to_numpy(vh).view(np.uint32).reshape(ns, R, nbin)
    return tuple(got)


def _block(pkg, kind, R, F, nbin, Ts, ns):
    x, models, T0, tf = _case(kind, R, F, nbin, Ts, ns)
    blk = pkg.clFolder(*GPU_ARGS, R, F, nbin, Ts, models)
    blk.set_sample(T0)
    return blk


def _both_routes(blk, own):
    """yields the route name for the handle's own route and, where that is the bin-owner one, again under set_generic"""
    blk.set_generic(False)
    assert blk.route().startswith(own + " ")
    yield own
    if own == "bins":
        blk.set_generic(True)
        assert blk.route().startswith("generic ")
        yield "generic (forced)"
        blk.set_generic(False)


@pytest.mark.parametrize("R,F,nbin,Ts,ns", BINS + GENERIC)
def test_route_strings(gpu, pkg, R, F, nbin, Ts, ns):
    blk = pkg.clFolder(*GPU_ARGS, R, F, nbin, Ts, np.zeros((R, 3), np.uint64))
    tail = " R=%d F=%d nbin=%d Ts=%d" % (R, F, nbin, Ts)
    assert blk.route() == _route_of(F) + tail and blk.subint_len == Ts == pkg.lib().mi355_fold_subint_len(blk._h)
    blk.set_generic(True)
    assert blk.route() == "generic" + tail
    blk.set_generic(False)
    assert blk.route() == _route_of(F) + tail
    assert (blk.floats_per_sample(), blk.floats_per_subint(), blk.hits_per_subint()) == (R * F, R * nbin * F, R * nbin)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,F,nbin,Ts,ns", BINS + GENERIC)
def test_equals_the_reference(gpu, pkg, R, F, nbin, Ts, ns, kind):
    """every shape and every kind of model and input, on the shape's own route and, for the bin-owner shapes, again under set_generic"""
    x, models, T0, tf = _case(kind, R, F, nbin, Ts, ns)
    want = _want(kind, R, F, nbin, Ts, ns)
    blk = _block(pkg, kind, R, F, nbin, Ts, ns)
    for r in _both_routes(blk, _route_of(F)):
        blk.set_sample(T0)
        got = _run(blk, x, tf, finite=(kind != "nan"))
        assert _same(got, want), r
        assert blk.sample() == (T0 + x.shape[0]) & M64
    assert int(want[1].sum()) == (x.shape[0] * R if tf is None else int((tf == 0).sum()))
    if kind == "nu0":
        assert (want[1] != 0).sum() == ns * R           # everything of a row in one bin
    if nbin == 4096:
        assert (want[1] == 0).mean() > 0.99 and not _bits(want[0][want[1] == 0]).any()   # empty bins are +0.0f
    if kind in ("nudot+", "nudot-"):
        # the boundaries move inside a sub-integration: the bins leave those of the same phase and frequency at T0 without nudot
        phi0, nu, nudot = (int(v) for v in models[0])
        lin = ref.bins(ref.words(ref.phi(models[0], T0), nu + nudot * T0, 0), 0, Ts, nbin)
        assert (lin != ref.bins(models[0], T0, Ts, nbin)).any()
    if kind == "nan":
        n = x.shape[0]
        j, r0, f0 = (n // 3) // Ts, R // 2, F // 2
        assert np.isnan(want[0]).sum() == 1 and np.isnan(want[0][j, r0, ref.bin_of(models[r0], T0 + n // 3, nbin), f0])
        assert np.isinf(want[0]).sum() == 1
    if kind == "negzero":
        assert not _bits(want[0][:, R - 1, :, F // 3]).any()   # -0.0f folds to +0.0f, in empty and in filled bins alike
    if kind == "flags":
        assert tf.any() and int(want[1].sum()) < x.shape[0] * R


@pytest.mark.parametrize("R,F,nbin,Ts", [(2, 256, 16, 64), (3, 320, 7, 48), (3, 52, 7, 48)])
def test_one_call_four_calls_and_skip(gpu, pkg, R, F, nbin, Ts):
    """four sub-integrations in one call, in four calls, and the first and the last alone with skip() over the two between"""
    kind, ns = "nudot-", 4
    x, models, T0, tf = _case(kind, R, F, nbin, Ts, ns)
    want = _want(kind, R, F, nbin, Ts, ns)
    blk = _block(pkg, kind, R, F, nbin, Ts, ns)
    for r in _both_routes(blk, _route_of(F)):
        blk.set_sample(T0)
        assert _same(_run(blk, x), want), r
        blk.set_sample(T0)
        for j in range(ns):
            got = _run(blk, x[j * Ts:(j + 1) * Ts])
            assert _same(got, (want[0][j], want[1][j])), (r, j)
        blk.set_sample(T0)
        assert _same(_run(blk, x[:Ts]), (want[0][0], want[1][0])), r
        blk.skip(2 * Ts)
        assert blk.sample() == T0 + 3 * Ts
        assert _same(_run(blk, x[3 * Ts:]), (want[0][3], want[1][3])), r


@pytest.mark.parametrize("R,F,nbin,Ts,ns", [(2, 256, 16, 64, 2), (3, 320, 7, 48, 2), (1, 64, 2, 16, 3), (3, 52, 7, 48, 2)])
def test_alignment(gpu, pkg, R, F, nbin, Ts, ns):
    """in and out 4, 8 and 12 bytes past a 16-byte boundary; with and without hits"""
    x, models, T0, tf = _case("plain", R, F, nbin, Ts, ns)
    want = _want("plain", R, F, nbin, Ts, ns)
    blk = _block(pkg, "plain", R, F, nbin, Ts, ns)
    for r in _both_routes(blk, _route_of(F)):
        for in_off, out_off in ((1, 0), (0, 1), (1, 1), (2, 3), (3, 2)):
            blk.set_sample(T0)
            assert _same(_run(blk, x, in_off=in_off, out_off=out_off), want), (r, in_off, out_off)
        blk.set_sample(T0)
        assert _same(_run(blk, x, hits=False)[:1], want[:1]), r


def test_set_models_between_calls(gpu, pkg):
    """two calls enqueued back to back with a set_models between them: the first uses the old table entirely, the second the new one;
    a refused update changes nothing"""
    import torch
    R, F, nbin, Ts, ns = 2, 256, 16, 64, 2
    x, m1, _, _ = _case("plain", R, F, nbin, Ts, ns)
    m2 = _models("nudot+", R, nbin, Ts)
    n = ns * Ts
    w1 = ref.fold(x, m1, 0, nbin, Ts)
    w2 = ref.fold(x, m2, n, nbin, Ts)
    blk = pkg.clFolder(*GPU_ARGS, R, F, nbin, Ts, m1)
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    for r in _both_routes(blk, "bins"):
        blk.set_sample(0)
        blk.set_models(m1)
        outs = [[torch.full((ns * R * nbin * F,), float("nan"), device="cuda"), torch.full((ns * R * nbin,), -1, dtype=torch.int32, device="cuda")]
                for _ in range(2)]
        torch.cuda.synchronize()
        blk.work_device(ns, [d_x], outs[0])
        blk.set_models(m2)
        blk.work_device(ns, [d_x], outs[1])
        torch.cuda.synchronize()
        for o, w in zip(outs, (w1, w2)):
            assert _same((o[0].cpu().numpy(), o[1].cpu().numpy()), w), r
        assert np.array_equal(blk.models(), m2)
    with pytest.raises(ValueError):
        blk.set_models(m2[:-1])
    with pytest.raises(TypeError):
        blk.set_models(m2.astype(np.int64))
    assert pkg.lib().mi355_fold_set_models(blk._h, None) == -1
    assert np.array_equal(blk.models(), m2)  # a refused update changes nothing
    blk.set_sample(n)
    assert _same(_run(blk, x), w2)


@pytest.mark.parametrize("R,F,nbin,Ts,ns", [(2, 256, 16, 64, 2), (3, 52, 7, 48, 2)])
def test_host_work_equals_the_reference(gpu, pkg, R, F, nbin, Ts, ns):
    x, models, T0, tf = _case("flags", R, F, nbin, Ts, ns)
    want = _want("flags", R, F, nbin, Ts, ns)
    blk = _block(pkg, "flags", R, F, nbin, Ts, ns)
    for r in _both_routes(blk, _route_of(F)):
        blk.set_sample(T0)
        assert _same(blk.fold(x, tf, hits=True), want), r
        assert blk.sample() == T0 + ns * Ts
        blk.set_sample(T0)
        assert _same((blk.fold(x, tf),), want), r
    with pytest.raises(ValueError):
        blk.work(ns, [x.reshape(-1)[:-1]], [np.empty_like(want[0])])
    with pytest.raises(pkg.Mi355Error):
        pkg.check(pkg.lib().mi355_fold_work(blk._h, Ts + 1, C.c_void_p(x.ctypes.data), None, C.c_void_p(np.empty_like(want[0]).ctypes.data), None),
                  "mi355_fold_work")


def test_host_work_in_pieces(gpu, pkg):
    """sub-integrations of 4096 x 2 x 256 floats = 8 MiB: work() sends the 3 sub-integrations as 3 pieces, each at its own T"""
    R, F, nbin, Ts, ns = 2, 256, 5, 4096, 3
    x, models, T0, tf = _case("nudot+", R, F, nbin, Ts, ns)
    want = _want("nudot+", R, F, nbin, Ts, ns)
    blk = _block(pkg, "nudot+", R, F, nbin, Ts, ns)
    assert blk.route().startswith("bins ")
    assert _same(blk.fold(x, hits=True), want)
    assert blk.sample() == T0 + ns * Ts


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    R, F, nbin, Ts = 2, 8, 4, 16  # one sub-integration: 1024 bytes of samples, 256 bytes of archive, 32 of hits, 32 tflags
    blk = pkg.clFolder(*GPU_ARGS, R, F, nbin, Ts, np.zeros((R, 3), np.uint64))
    blk.set_sample(77)
    L, h = pkg.lib(), blk._h
    buf = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    p = buf.data_ptr()
    vp = C.c_void_p
    W = L.mi355_fold_work_dev
    assert W(h, 16, vp(p + 2), None, vp(p + 4096), None, None) == -1                  # in not 4-byte aligned
    assert W(h, 16, vp(p), None, vp(p + 4096 + 2), None, None) == -1                  # out not 4-byte aligned
    assert W(h, 16, vp(p), None, vp(p + 4096), vp(p + 8192 + 2), None) == -1          # hits not 4-byte aligned
    assert W(h, 16, vp(p), None, vp(p), None, None) == -1                             # out is in: there is no in-place fold
    assert W(h, 16, vp(p), None, vp(p + 1020), None, None) == -1                      # out starts inside in
    assert W(h, 16, vp(p + 252), None, vp(p), None, None) == -1                       # in starts inside out
    assert W(h, 32, vp(p + 508), None, vp(p), None, None) == -1                       # two sub-integrations: 512 bytes of archive
    assert W(h, 16, vp(p), vp(p + 1023), vp(p + 4096), None, None) == -1              # tflags inside in
    assert W(h, 16, vp(p), vp(p + 4096 + 255), vp(p + 4096), None, None) == -1        # tflags inside out
    assert W(h, 16, vp(p), None, vp(p + 4096), vp(p + 4096 + 252), None) == -1        # hits inside out
    assert W(h, 16, vp(p), vp(p + 8192 + 31), vp(p + 4096), vp(p + 8192), None) == -1 # tflags inside hits
    assert W(h, 16, vp(p), None, vp(p + 4096), vp(p + 1020), None) == -1              # hits inside in
    assert W(h, 17, vp(p), None, vp(p + 4096), None, None) == -1                      # n is no multiple of Ts
    assert W(h, -16, vp(p), None, vp(p + 4096), None, None) == -1
    assert W(h, 16, None, None, vp(p + 4096), None, None) == -1
    assert W(h, 16, vp(p), None, None, None, None) == -1
    assert W(h, ((1 << 40) // 64 // 16 + 1) * 16, vp(p), None, vp(p + (1 << 50)), None, None) == -3  # samples of 64 bytes pass 2^40
    assert L.mi355_fold_work(h, 16, vp(p + 2), None, vp(p + 4096), None) == -1
    assert L.mi355_fold_skip(h, -1) == -1
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0  # nothing was launched
    assert blk.sample() == 77         # and the stream did not move
    # the archive of a call may pass 2^40 bytes while its input does not
    big = pkg.clFolder(*GPU_ARGS, 64, 1024, 4096, 16, np.zeros((64, 3), np.uint64))
    assert W(big._h, 16 * 1025, vp(p), None, vp(p + (1 << 50)), None, None) == -3


def test_zero_samples_is_a_no_op(gpu, pkg):
    import torch
    blk = pkg.clFolder(*GPU_ARGS, 2, 8, 4, 16, np.zeros((2, 3), np.uint64))
    out = torch.full((256,), 7.0, dtype=torch.float32, device="cuda")
    assert pkg.lib().mi355_fold_work_dev(blk._h, 0, None, None, C.c_void_p(out.data_ptr()), None, None) == 0
    assert pkg.lib().mi355_fold_work(blk._h, 0, None, None, None, None) == 0
    assert blk.work_device(0, [out], [out]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and blk.sample() == 0


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, Ts items in per item out, the optional flag and hit streams"""
    mod = _pybind()
    R, F, nbin, Ts, ns = 2, 256, 16, 64, 2
    x, models, T0, tf = _case("flags", R, F, nbin, Ts, ns)
    want = _want("flags", R, F, nbin, Ts, ns)
    fo = mod.clFolder(*GPU_ARGS, R, F, nbin, Ts, models.reshape(-1))
    assert fo.decimation() == Ts and fo.history() == 1 and fo.subint_len() == Ts and fo.nbin() == nbin and fo.route().startswith("bins ")
    assert np.array_equal(fo.models(), models.reshape(-1)) and fo.sample() == 0
    for generic in (False, True):
        fo.set_generic(generic)
        assert fo.route().startswith("generic " if generic else "bins ")
        fo.set_sample(T0)
        y = np.full(want[0].shape, np.nan, np.float32)
        h = np.full(want[1].shape, 0xFFFFFFFF, np.uint32)
        assert fo.work(ns, [x, tf], [y, h]) == ns
        assert _same((y, h), want) and fo.sample() == T0 + ns * Ts
    plain = ref.fold(x, models, 5, nbin, Ts)
    fo.set_sample(0)
    fo.skip(5)
    y = np.full(want[0].shape, np.nan, np.float32)
    assert fo.work(ns, [x], [y]) == ns and _same((y,), plain)
    with pytest.raises(ValueError):
        fo.set_models(models.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        fo.work(ns, [x.reshape(-1)[:-1]], [y])  # one float fewer than the call reads
    with pytest.raises(ValueError):
        mod.clFolder(*GPU_ARGS, R, F, nbin, 40, models.reshape(-1))


def test_cli_row(gpu):
    """test-clenabled-mi355 --fold-only prints the checksum of a small run on generated samples"""
    r = subprocess.run([CLI, "--fold-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    R, F, nbin, Ts, ns = 2, 256, 8, 32, 3
    n = ns * Ts
    state, vals = 12345, np.empty(n * R * F, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    x = (vals + 1).astype(np.float32).reshape(n, R, F)
    models = np.stack([ref.words(0, (1 << 64) // 9, 0), ref.words(1 << 62, (1 << 64) // 5 + 3, -(1 << 44))])
    out, hits = ref.fold(x, models, 1000, nbin, Ts)
    u = np.uint64

    def wsum(a, m):
        a = a.reshape(-1).astype(u)
        return int(((np.arange(a.size, dtype=u) % u(m) + u(1)) * a).sum(dtype=u))

    want = (wsum(out.view(np.uint32), 7) + wsum(hits, 5)) % (1 << 64)
    assert re.search(r"^clFolder checksum (\d+)$", r.stdout, re.M).group(1) == str(want), r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clFolder (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout


def test_beamformer_and_cleaner_feed_the_folder(gpu, pkg):
    """int8 frames of seeded noise with louder voltages wherever the pulsar's phase is in bin b0 -> clBeamformer POWER (stokes_i) ->
    clFilterbankCleaner (zero-DM off, no limits; its tflags go to the folder as they stand) -> clFolder, all on the device: equal to
    beamform_ref, fbclean_ref and fold_ref chained, bit for bit, on both routes of the folder; the channel-summed profile of beam 0
    peaks in the bin fold_bins predicts"""
    import torch
    R, F, S, npol, Ti, Tb = 2, 256, 4, 2, 4, 32
    nbin, Ts, ns, T0, b0 = 8, 64, 2, 5000, 5
    n = ns * Ts
    model = pkg.fold_model(8.3e-3, 0.0, 1e-3, 0.1)                  # 8.3 samples per turn
    models = np.stack([model, ref.words(0, (1 << 64) // 11, 1 << 40)])
    bins = pkg.fold_bins(model, T0, n, nbin)
    assert np.array_equal(bins, ref.bins(model, T0, n, nbin)) and (bins == b0).sum() >= 8
    rng = np.random.default_rng(2026)
    frames = rng.integers(-8, 9, size=(n * Ti, S, F, npol, 2), dtype=np.int8)
    on = np.repeat(bins == b0, Ti)
    frames[on] = rng.integers(-24, 25, size=(int(on.sum()), S, F, npol, 2), dtype=np.int8)
    w = np.zeros((F, npol, R, S, 2), np.int8)
    w[:, :, 0, :, 0] = 1
    w[:, :, 1] = rng.integers(-20, 21, size=(F, npol, S, 2), dtype=np.int8)
    power = beamform_ref.power(frames, w, Ti, True)                   # [t][beam][chan] float32
    clean, cf, tf, st = fbclean_ref.clean(power, Tb, float(Ti * npol), -np.inf, np.inf, np.inf, 0)
    assert not tf.any() and not cf.any()
    want = ref.fold(clean, models, T0, nbin, Ts, tf)
    bf = pkg.clBeamformer(*GPU_ARGS, beamform_ref.POWER, npol, S, F, R, Ti, True, w)
    fc = pkg.clFilterbankCleaner(*GPU_ARGS, R, F, Tb, float(Ti * npol), -np.inf, np.inf, np.inf, 0)
    fo = pkg.clFolder(*GPU_ARGS, R, F, nbin, Ts, models)
    assert bf.out_items_per_unit() == fc.floats_per_sample() == fo.floats_per_sample() == R * F
    d_power = torch.full((n * R * F,), float("nan"), dtype=torch.float32, device="cuda")
    d_tf = torch.full((n * R,), -1, dtype=torch.int8, device="cuda")
    assert bf.work_device(n, [torch.from_numpy(frames.reshape(-1)).cuda()], [d_power]) == n
    assert fc.work_device(n, [d_power], [d_power, None, d_tf]) == n
    for r in _both_routes(fo, "bins"):
        fo.set_sample(T0)
        wo, vo = guarded.guarded_output(ns * R * nbin * F, np.float32, guarded.pad_items(4, R * F), 0, "cuda")
        wh, vh = guarded.guarded_output(ns * R * nbin, np.int32, guarded.pad_items(4, R * nbin), 0, "cuda")
        assert fo.work_device(ns, [d_power, d_tf], [vo, vh]) == ns
        torch.cuda.synchronize()
        guarded.check_guards(wo, vo, "archive")
        guarded.check_guards(wh, vh, "hits")
        assert np.array_equal(d_power.cpu().numpy().view(np.uint32), _bits(clean)), r
        got = (guarded.to_numpy(vo).reshape(want[0].shape), guarded.to_numpy(vh).view(np.uint32).reshape(want[1].shape))
        assert _same(got, want), r
        profile = got[0][:, 0].astype(np.float64).sum(axis=(0, 2))     # beam 0: [bin]
        assert int(np.argmax(profile)) == b0, (r, profile)
