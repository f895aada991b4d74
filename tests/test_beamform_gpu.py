"""GPU: clBeamformer against tests/beamform_ref.py (numpy integer arithmetic).  Both modes are integer-exact, so every comparison is
array_equal: there is no tolerance anywhere.  Inputs are seeded full-range int8 (-128 included), weights seeded in -127 .. 127; every
device call runs on guard-banded buffers (tests/guarded.py) whose output interior is NaN before the call.

Routes, as csrc/beamform.hip states them:
  mfma     F npol a multiple of 8 and S <= 256: k_bf_mfma<K blocks, beam tiles, mode>
  generic  everything else, every handle under set_generic(True), and a call whose `in` is not 16-byte aligned: k_bf_gen_v / k_bf_gen_p

On an MI355X the file takes 3.3 s (24 tests).
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
import beamform_ref as ref
import guarded

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")

# (S, B, F, npol, T frames, route)
FIXED = [
    (64, 64, 8, 1, 64, "mfma"),
    (64, 16, 16, 2, 80, "mfma"),
    (16, 16, 8, 1, 33, "mfma"),      # K padded 16 -> 64; T not a multiple of any tile
    (20, 5, 8, 2, 17, "mfma"),       # S and B off the 16-grid
    (256, 128, 8, 1, 16, "mfma"),    # four K blocks of 64
    (4, 1, 8, 1, 1, "mfma"),
    (3, 2, 5, 1, 9, "generic"),
    (512, 3, 4, 1, 4, "generic"),    # extremes: 16 646 144 arrives exactly
]


@functools.lru_cache(maxsize=None)
def _data(S, B, F, npol, T, seed=0, extreme=False):
    if extreme:
        return ref.extremes(T, S, F, npol, B)
    rng = np.random.default_rng(1000 + seed + S * 7 + B * 11 + F * 13 + npol * 17 + T * 19)
    return ref.frames(rng, T, S, F, npol), ref.weights(rng, S, F, npol, B)


@functools.lru_cache(maxsize=None)
def _want_v(S, B, F, npol, T, seed=0, extreme=False):
    x, w = _data(S, B, F, npol, T, seed, extreme)
    y = ref.voltage(x, w)
    y.setflags(write=False)
    return y


def _run(blk, x, nunits, in_off=0, out_off=0):
    """work_device on guard-banded buffers: `x` the int8 frames of the call; offsets in items of the buffer's dtype past 16 bytes"""
    import torch
    n_out = nunits * blk.out_items_per_unit()
    dt = np.complex64 if blk.mode == ref.VOLTAGE else np.float32
    xin = np.ascontiguousarray(x).reshape(-1)[:nunits * blk.frames_per_unit() * blk.frame_bytes()]
    wi, vi = guarded.guarded_input(xin, guarded.pad_items(1, blk.frame_bytes()), in_off, "cuda")
    wo, vo = guarded.guarded_output(n_out, dt, guarded.pad_items(np.dtype(dt).itemsize, blk.out_items_per_unit()), out_off, "cuda")
    assert blk.work_device(nunits, [vi], [vo]) == nunits
    torch.cuda.synchronize()
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "output")
    return guarded.to_numpy(vo)


def _both_routes(blk, expect_route):
    """yields the route names after asserting them: the geometry's own route, then the forced generic one"""
    assert blk.route().startswith(expect_route), blk.route()
    yield blk.route()
    blk.set_generic(True)
    assert blk.route().startswith("generic"), blk.route()
    yield blk.route()
    blk.set_generic(False)
    assert blk.route().startswith(expect_route)


@pytest.mark.parametrize("S,B,F,npol,T,route", FIXED)
def test_voltage_fixed(gpu, pkg, S, B, F, npol, T, route):
    extreme = S == 512
    x, w = _data(S, B, F, npol, T, 0, extreme)
    want = _want_v(S, B, F, npol, T, 0, extreme).reshape(-1)
    if extreme:
        assert want.real.max() == 16646144.0 and np.all(want.real == 16646144.0) and np.all(want.imag == 0.0)
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B, 1, False, w)
    assert (blk.frame_bytes(), blk.frames_per_unit(), blk.out_bytes_per_unit()) == ref.plan(ref.VOLTAGE, npol, S, F, B)
    for r in _both_routes(blk, route):
        got = _run(blk, x, T)
        assert np.array_equal(got, want), (r, int(np.argmax(got != want)))


@pytest.mark.parametrize("stokes", [False, True])
def test_power_windows(gpu, pkg, stokes):
    S, B, F, npol, Ti, W = 64, 64, 8, 2, 32, 3
    x, w = _data(S, B, F, npol, Ti * W, 1)
    want = ref.power(x, w, Ti, stokes).reshape(-1)
    blk = pkg.clBeamformer(*GPU_ARGS, ref.POWER, npol, S, F, B, Ti, stokes, w)
    assert (blk.frame_bytes(), blk.frames_per_unit(), blk.out_bytes_per_unit()) == ref.plan(ref.POWER, npol, S, F, B, Ti, stokes)
    outs = []
    for r in _both_routes(blk, "mfma"):
        outs.append(_run(blk, x, W))
        assert np.array_equal(outs[-1], want), r
    # split invariance: 3 windows as 1 + 2
    fb = blk.frame_bytes() * Ti
    flat = x.reshape(-1)
    parts = np.concatenate([_run(blk, flat[:fb], 1), _run(blk, flat[fb:], 2)])
    assert np.array_equal(parts, want)


def _near_extremes(T, S, F, npol, B):
    """the extremes with one weight and one sample a step inside, so that re is odd and the window sum has more than 24 significant bits"""
    x, w = ref.extremes(T, S, F, npol, B)
    x, w = x.copy(), w.copy()
    w[..., 0, 1] = 126
    x[:, 1, ..., 0] = -127
    return x, w


@pytest.mark.parametrize("near", [False, True])
def test_power_long_window_at_the_extremes(gpu, pkg, near):
    """Ti = 4096, every product at (near) full scale: an int64 sum far above 2^53; the `near` form needs rounding to float32"""
    S, B, F, npol, Ti = 16, 16, 8, 1, 4096
    x, w = _near_extremes(Ti, S, F, npol, B) if near else ref.extremes(Ti, S, F, npol, B)
    exact = ref.power_int(x, w, Ti)
    want = exact.astype(np.float32).reshape(-1)
    if near:  # the integer sum is not representable in float32, so the conversion really rounds
        assert np.all(want.astype(np.float64).astype(np.int64).reshape(exact.shape) != exact)
        assert int(exact.max()) > 1 << 24
    blk = pkg.clBeamformer(*GPU_ARGS, ref.POWER, npol, S, F, B, Ti, False, w)
    for r in _both_routes(blk, "mfma"):
        assert np.array_equal(_run(blk, x, 1), want), r


def test_power_integration_one(gpu, pkg):
    S, B, F, npol, W = 20, 5, 8, 2, 9
    x, w = _data(S, B, F, npol, W, 2)
    for stokes in (False, True):
        want = ref.power(x, w, 1, stokes).reshape(-1)
        blk = pkg.clBeamformer(*GPU_ARGS, ref.POWER, npol, S, F, B, 1, stokes, w)
        for r in _both_routes(blk, "mfma"):
            assert np.array_equal(_run(blk, x, W), want), (r, stokes)


def test_voltage_split_invariance(gpu, pkg):
    S, B, F, npol, T = 64, 16, 16, 2, 80
    x, w = _data(S, B, F, npol, T)
    want = _want_v(S, B, F, npol, T).reshape(-1)
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B, 1, False, w)
    fb = blk.frame_bytes()
    flat = x.reshape(-1)
    for r in _both_routes(blk, "mfma"):
        parts, t0 = [], 0
        for n in (1, 7, 64, 8):
            parts.append(_run(blk, flat[t0 * fb:(t0 + n) * fb], n))
            t0 += n
        assert np.array_equal(np.concatenate(parts), want), r


@pytest.mark.parametrize("mode", [ref.VOLTAGE, ref.POWER])
def test_alignment(gpu, pkg, mode):
    """`in` 2 and 8 bytes past a 16-byte boundary (the generic kernel serves that call), `out` 8 (VOLTAGE) / 4 (POWER) bytes past one:
    the bits of the aligned call.  S = 20: the K padding must not read past the frames, which end where the guard band starts."""
    S, B, F, npol, Ti, W = 20, 5, 8, 2, (1 if mode == ref.VOLTAGE else 4), 5
    x, w = _data(S, B, F, npol, Ti * W, 3)
    want = (ref.voltage(x, w) if mode == ref.VOLTAGE else ref.power(x, w, Ti)).reshape(-1)
    blk = pkg.clBeamformer(*GPU_ARGS, mode, npol, S, F, B, Ti, False, w)
    for r in _both_routes(blk, "mfma"):
        for in_off, out_off in ((0, 0), (2, 0), (8, 0), (0, 1), (2, 1), (6, 3)):
            assert np.array_equal(_run(blk, x, W, in_off, out_off), want), (r, in_off, out_off)


def test_misaligned_and_overlapping_buffers_are_refused(gpu, pkg):
    import torch
    S, B, F, npol = 4, 2, 8, 1
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B)
    L, h = pkg.lib(), blk._h
    buf = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    p = buf.data_ptr()
    assert L.mi355_beamform_work_dev(h, 1, C.c_void_p(p + 1), C.c_void_p(p + 4096), None) == -1      # in not 2-byte aligned
    assert L.mi355_beamform_work_dev(h, 1, C.c_void_p(p), C.c_void_p(p + 4096 + 4), None) == -1      # out not 8-byte aligned
    assert L.mi355_beamform_work_dev(h, 1, C.c_void_p(p), C.c_void_p(p + 56), None) == -1            # overlap: the frame is 64 bytes
    assert L.mi355_beamform_work_dev(h, 1, None, C.c_void_p(p), None) == -1
    assert L.mi355_beamform_work_dev(h, -1, C.c_void_p(p), C.c_void_p(p + 4096), None) == -1
    assert L.mi355_beamform_work_dev(h, (1 << 40) // 64 + 1, C.c_void_p(p), C.c_void_p(p + 4096), None) == -3
    pw = pkg.clBeamformer(*GPU_ARGS, ref.POWER, npol, S, F, B, 2)
    assert L.mi355_beamform_work_dev(pw._h, 1, C.c_void_p(p), C.c_void_p(p + 4096 + 2), None) == -1  # out not 4-byte aligned
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0  # nothing was launched


def test_zero_units_is_a_no_op(gpu, pkg):
    import torch
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, 1, 4, 8, 2)
    out = torch.full((256,), 7.0, dtype=torch.float32, device="cuda")
    assert pkg.lib().mi355_beamform_work_dev(blk._h, 0, None, C.c_void_p(out.data_ptr()), None) == 0
    assert pkg.lib().mi355_beamform_work(blk._h, 0, None, None) == 0
    assert blk.work_device(0, [out], [out]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_set_beam_weights_changes_one_beam(gpu, pkg):
    S, B, F, npol, T = 20, 5, 8, 2, 17
    x, w = _data(S, B, F, npol, T)
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B, 1, False, w)
    assert np.array_equal(blk.weights(), w)
    rng = np.random.default_rng(5)
    wb = rng.integers(-127, 128, size=(F, npol, S, 2), dtype=np.int8)
    w2 = w.copy()
    w2[:, :, 3] = wb
    for r in _both_routes(blk, "mfma"):
        blk.set_weights(w)
        before = _run(blk, x, T).reshape(T, B, F, npol)
        blk.set_beam_weights(3, wb)
        assert np.array_equal(blk.weights(), w2)
        after = _run(blk, x, T).reshape(T, B, F, npol)
        assert np.array_equal(after, ref.voltage(x, w2)), r
        others = [b for b in range(B) if b != 3]
        assert np.array_equal(after[:, others], before[:, others]) and not np.array_equal(after[:, 3], before[:, 3])
    with pytest.raises(pkg.Mi355Error):
        blk.set_beam_weights(B, wb)
    with pytest.raises(pkg.Mi355Error):
        blk.set_beam_weights(-1, wb)
    bad = wb.copy()
    bad[0, 0, 0, 0] = -128
    with pytest.raises(pkg.Mi355Error):
        blk.set_beam_weights(0, bad)
    assert np.array_equal(blk.weights(), w2)  # a refused update changes nothing


def test_set_weights_between_enqueued_calls(gpu, pkg):
    """two work_dev calls on one stream with set_weights between them and no synchronisation: old weights entirely, then new entirely"""
    import torch
    S, B, F, npol, T = 64, 16, 16, 2, 80
    x, w = _data(S, B, F, npol, T)
    _, w_new = _data(S, B, F, npol, T, 9)
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B, 1, False, w)
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    for r in _both_routes(blk, "mfma"):
        blk.set_weights(w)
        o1 = torch.full((T * B * F * npol,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda")
        o2 = torch.full_like(o1, complex(np.nan, np.nan))
        torch.cuda.synchronize()
        blk.work_device(T, [d_x], [o1])
        blk.set_weights(w_new)
        blk.work_device(T, [d_x], [o2])
        torch.cuda.synchronize()
        assert np.array_equal(o1.cpu().numpy(), _want_v(S, B, F, npol, T).reshape(-1)), r
        assert np.array_equal(o2.cpu().numpy(), ref.voltage(x, w_new).reshape(-1)), r


def test_set_weights_with_two_streams_on_one_handle(gpu, pkg):
    """weights 1 read on stream A, then on stream B; weights 2 on B, weights 3 on A; one synchronisation at the end.  A weight table is
    released only behind its readers on every stream, not behind the stream that happened to read it last."""
    import torch
    S, B, F, npol, T = 4, 1, 8, 1, 1
    reps = 512  # T frames, repeated: a few thousand items per call
    x, w1 = _data(S, B, F, npol, T)
    ws = [w1, _data(S, B, F, npol, T, 9)[1], _data(S, B, F, npol, T, 10)[1]]
    x = np.ascontiguousarray(np.concatenate([x] * reps))
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B, 1, False, w1)
    assert blk.route().startswith("mfma")
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    outs = [torch.full((T * reps * B * F * npol,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(4)]
    sA, sB = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(sA):
        blk.work_device(T * reps, [d_x], [outs[0]])
    with torch.cuda.stream(sB):
        blk.work_device(T * reps, [d_x], [outs[1]])
    blk.set_weights(ws[1])
    with torch.cuda.stream(sB):
        blk.work_device(T * reps, [d_x], [outs[2]])
    blk.set_weights(ws[2])
    with torch.cuda.stream(sA):
        blk.work_device(T * reps, [d_x], [outs[3]])
    torch.cuda.synchronize()
    for i, w in enumerate((ws[0], ws[0], ws[1], ws[2])):
        assert np.array_equal(outs[i].cpu().numpy(), ref.voltage(x, w).reshape(-1)), i


def test_host_work_equals_device_work(gpu, pkg):
    S, B, F, npol, T = 20, 5, 8, 2, 17
    x, w = _data(S, B, F, npol, T)
    blk = pkg.clBeamformer(*GPU_ARGS, ref.VOLTAGE, npol, S, F, B, 1, False, w)
    y = np.full(T * B * F * npol, np.nan + 0j, np.complex64)
    assert blk.work(T, [x], [y]) == T
    assert np.array_equal(y, _run(blk, x, T)) and np.array_equal(y, _want_v(S, B, F, npol, T).reshape(-1))
    Ti, W = 4, 4
    pw = pkg.clBeamformer(*GPU_ARGS, ref.POWER, npol, S, F, B, Ti, True, w)
    p = np.full(W * B * F, np.nan, np.float32)
    assert pw.work(W, [x[:Ti * W]], [p]) == W
    assert np.array_equal(p, _run(pw, x[:Ti * W], W)) and np.array_equal(p, ref.power(x[:Ti * W], w, Ti, True).reshape(-1))
    with pytest.raises(ValueError):
        blk.work(T + 1, [x], [y])


def _sweep_geometries(n=60, seed=2024):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cols = int(rng.choice([8, 16, 24, 32])) if rng.random() < 0.75 else int(rng.integers(1, 33))
        npol = int(rng.integers(1, 3)) if cols % 2 == 0 else 1
        mode = int(rng.integers(0, 2))
        Ti = int(rng.integers(1, 9)) if mode == ref.POWER else 1
        units = int(rng.integers(1, 40 // Ti + 1))
        stokes = bool(mode == ref.POWER and npol == 2 and rng.random() < 0.5)
        out.append((int(rng.integers(1, 97)), int(rng.integers(1, 41)), cols // npol, npol, mode, Ti, units, stokes, int(rng.integers(1 << 30))))
    return out


def test_random_sweep(gpu, pkg):
    """60 seeded geometries, S <= 96, B <= 40, F npol <= 32, T <= 40, both modes: the reference's bits on both routes"""
    generic = 0
    geos = _sweep_geometries()
    for S, B, F, npol, mode, Ti, units, stokes, seed in geos:
        rng = np.random.default_rng(seed)
        x, w = ref.frames(rng, Ti * units, S, F, npol), ref.weights(rng, S, F, npol, B)
        want = (ref.voltage(x, w) if mode == ref.VOLTAGE else ref.power(x, w, Ti, stokes)).reshape(-1)
        blk = pkg.clBeamformer(*GPU_ARGS, mode, npol, S, F, B, Ti, stokes, w)
        expect = "mfma" if (F * npol) % 8 == 0 else "generic"
        generic += expect == "generic"
        got = [_run(blk, x, units) for _ in _both_routes(blk, expect)]
        geo = (S, B, F, npol, mode, Ti, units, stokes)
        assert np.array_equal(got[0], want), geo
        assert np.array_equal(got[1], want) and np.array_equal(got[0], got[1]), geo
        blk.stop()
    assert 0 < generic <= len(geos) // 2, generic


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, frames in, units out; decimation by the integration in POWER mode"""
    mod = _pybind()
    S, B, F, npol, T = 20, 5, 8, 2, 17
    x, w = _data(S, B, F, npol, T)
    bf = mod.clBeamformer(*GPU_ARGS, 0, npol, S, F, B, 1, False, w.reshape(-1))
    assert bf.decimation() == 1 and bf.num_beams() == B and bf.frame_bytes() == 2 * S * F * npol and bf.route().startswith("mfma")
    assert np.array_equal(bf.weights(), w.reshape(-1))
    y = np.full(T * B * F * npol, np.nan + 0j, np.complex64)
    assert bf.work(T, [x.reshape(-1)], [y]) == T
    assert np.array_equal(y, _want_v(S, B, F, npol, T).reshape(-1))
    print("pybind voltage checksum", int(y.real.astype(np.int64).sum() + y.imag.astype(np.int64).sum()))
    Ti, W = 4, 4
    pw = mod.clBeamformer(*GPU_ARGS, 1, npol, S, F, B, Ti, True)
    assert pw.decimation() == Ti and pw.out_bytes_per_unit() == 4 * B * F
    p = np.full(W * B * F, np.nan, np.float32)
    assert pw.work(W, [x.reshape(-1)], [p]) == W and np.all(p == 0.0)  # no weights yet: all zero
    pw.set_weights(w.reshape(-1))
    pw.set_generic(True)
    assert pw.route().startswith("generic")
    assert pw.work(W, [x.reshape(-1)], [p]) == W
    assert np.array_equal(p, ref.power(x[:Ti * W], w, Ti, True).reshape(-1))
    with pytest.raises(ValueError):
        pw.set_weights(w.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        pw.work(W + 1, [x.reshape(-1)], [p])  # 20 frames offered are 17
    with pytest.raises(ValueError):
        mod.clBeamformer(*GPU_ARGS, 0, npol, S, F, B, 2)  # integration must be 1 for VOLTAGE


def _lcg_bytes(n, state):
    out = np.empty(n, np.int64)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = state >> 24
    return (out - 256 * (out > 127)).astype(np.int8), state


def test_cli_row(gpu):
    """test-clenabled-mi355 --beamform-only prints checksums of a small voltage and a small Stokes-I run on generated frames"""
    r = subprocess.run([CLI, "--beamform-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    S, B, F, npol, T, Ti, W = 20, 5, 8, 2, 17, 4, 4
    xb, st = _lcg_bytes(T * S * F * npol * 2, 12345)
    wb, _ = _lcg_bytes(F * npol * B * S * 2, st)
    wb[wb == -128] = -127
    x, w = xb.reshape(T, S, F, npol, 2), wb.reshape(F, npol, B, S, 2)
    vr, vi = ref.voltage_int(x, w)
    i = np.arange(vr.size)
    vsum = int(((i % 7 + 1) * vr.reshape(-1)).sum() + ((i % 5 + 1) * vi.reshape(-1)).sum())
    p = ref.power(x[:Ti * W], w, Ti, True).reshape(-1).astype(np.float64)
    psum = float(((np.arange(p.size) % 7 + 1) * p).sum())
    assert re.search(r"^clBeamformer voltage checksum (-?\d+)$", r.stdout, re.M).group(1) == str(vsum), r.stdout
    assert re.search(r"^clBeamformer power checksum (\d+)$", r.stdout, re.M).group(1) == "%.0f" % psum, r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clBeamformer (")]
    assert len(rows) == 3 and all(l.rstrip().endswith("ok") for l in rows), r.stdout
