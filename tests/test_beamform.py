"""clBeamformer without a device: the sizes of mi355_beamform_plan, every argument error of the contract from _plan / _create with a NULL
context (which shows that the arguments are checked before the context is touched), and the self-checks of the yardstick
tests/beamform_ref.py.  The kernels are tested in tests/test_beamform_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import beamform_ref as ref


def _plan(L, mode, npol, S, F, B, Ti, stokes):
    fb, fpu, ob = C.c_longlong(-1), C.c_int(-1), C.c_longlong(-1)
    rc = L.mi355_beamform_plan(mode, npol, S, F, B, Ti, stokes, C.byref(fb), C.byref(fpu), C.byref(ob))
    return rc, (fb.value, fpu.value, ob.value), L.mi355_last_error().decode()


def _create(L, mode, npol, S, F, B, Ti, stokes, w=None, ctx=None):
    h = C.c_void_p(1)
    wp = None if w is None else C.c_void_p(w.ctypes.data)
    rc = L.mi355_beamform_create(ctx, mode, npol, S, F, B, Ti, stokes, wp, C.byref(h))
    assert rc != 0 and not h.value  # no handle comes back from a refused create
    return rc, L.mi355_last_error().decode()


def test_plan_sizes(pkg):
    L = pkg.lib()
    for npol, S, F, B in ((1, 64, 8, 64), (2, 64, 1024, 64), (2, 20, 5, 3), (1, 512, 1, 1024), (2, 1, 7, 1)):
        assert _plan(L, ref.VOLTAGE, npol, S, F, B, 1, 0)[:2] == (0, ref.plan(ref.VOLTAGE, npol, S, F, B))
        for Ti in (1, 32, 4096):
            assert _plan(L, ref.POWER, npol, S, F, B, Ti, 0)[:2] == (0, ref.plan(ref.POWER, npol, S, F, B, Ti))
            if npol == 2:
                assert _plan(L, ref.POWER, npol, S, F, B, Ti, 1)[:2] == (0, ref.plan(ref.POWER, npol, S, F, B, Ti, True))
    assert _plan(L, ref.VOLTAGE, 2, 64, 1024, 64, 1, 0)[1] == (262144, 1, 8 * 64 * 2048)
    assert _plan(L, ref.POWER, 2, 64, 1024, 64, 1024, 1)[1] == (262144, 1024, 4 * 64 * 1024)
    assert L.mi355_beamform_plan(0, 1, 4, 8, 2, 1, 0, None, None, None) == 0  # any output pointer may be NULL


BAD = [
    # (mode, npol, S, F, B, Ti, stokes), message
    ((2, 1, 4, 8, 2, 1, 0), "mode must be VOLTAGE (0) or POWER (1)"),
    ((-1, 1, 4, 8, 2, 1, 0), "mode must be VOLTAGE (0) or POWER (1)"),
    ((0, 0, 4, 8, 2, 1, 0), "npol must be 1 or 2"),
    ((0, 3, 4, 8, 2, 1, 0), "npol must be 1 or 2"),
    ((0, 1, 0, 8, 2, 1, 0), "num_inputs must be 1 .. 512"),
    ((0, 1, 513, 8, 2, 1, 0), "num_inputs must be 1 .. 512"),
    ((0, 1, 4, 0, 2, 1, 0), "num_channels must be >= 1"),
    ((0, 1, 4, 8, 0, 1, 0), "num_beams must be 1 .. 1024"),
    ((0, 1, 4, 8, 1025, 1, 0), "num_beams must be 1 .. 1024"),
    ((1, 1, 4, 8, 2, 0, 0), "integration must be 1 .. 4096"),
    ((1, 1, 4, 8, 2, 4097, 0), "integration must be 1 .. 4096"),
    ((0, 1, 4, 8, 2, 2, 0), "integration must be 1 in VOLTAGE mode"),
    ((1, 2, 4, 8, 2, 4, 2), "stokes_i must be 0 or 1"),
    ((1, 1, 4, 8, 2, 4, 1), "stokes_i needs POWER mode and npol = 2"),
    ((0, 2, 4, 8, 2, 1, 1), "stokes_i needs POWER mode and npol = 2"),
]


@pytest.mark.parametrize("args,msg", BAD)
def test_argument_errors_come_before_the_context(pkg, args, msg):
    L = pkg.lib()
    rc, sizes, err = _plan(L, *args)
    assert (rc, sizes, err) == (-1, (0, 0, 0), "invalid argument: " + msg)
    assert _create(L, *args) == (-1, "invalid argument: " + msg)                       # NULL context
    assert _create(L, *args, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: " + msg)  # an invalid one is never touched


def test_create_checks_weights_then_the_context(pkg):
    L = pkg.lib()
    S, F, B, npol = 4, 8, 2, 1
    w = np.zeros((F, npol, B, S, 2), np.int8)
    assert _create(L, 0, npol, S, F, B, 1, 0, w) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert _create(L, 0, npol, S, F, B, 1, 0, None) == (-1, "invalid argument: NULL context")
    for pos in ((0, 0, 0, 0, 0), (F - 1, 0, B - 1, S - 1, 1), (3, 0, 1, 2, 1)):
        bad = w.copy()
        bad[pos] = -128
        assert _create(L, 0, npol, S, F, B, 1, 0, bad, ctx=C.c_void_p(0xDEAD0000)) == \
            (-1, "invalid argument: a weight component of -128 (the range is -127 .. 127)")
    ok = np.full_like(w, -127)
    assert _create(L, 0, npol, S, F, B, 1, 0, ok) == (-1, "invalid argument: NULL context")
    assert L.mi355_beamform_create(None, 0, npol, S, F, B, 1, 0, None, None) == -1
    # a weight set above 2 GiB
    assert _plan(L, 0, 2, 512, 1 << 20, 1024, 1, 0)[0] == -3 and _create(L, 0, 2, 512, 1 << 20, 1024, 1, 0)[0] == -3


def test_null_handles(pkg):
    L = pkg.lib()
    assert L.mi355_beamform_set_weights(None, None) == -1 and L.mi355_beamform_set_beam_weights(None, 0, None) == -1
    assert L.mi355_beamform_get_weights(None, None, 0) == -1 and L.mi355_beamform_set_generic(None, 1) == -1
    assert L.mi355_beamform_num_beams(None) == -1 and L.mi355_beamform_frame_bytes(None) == -1
    assert L.mi355_beamform_out_bytes_per_unit(None) == -1
    assert L.mi355_beamform_work(None, 1, None, None) == -1 and L.mi355_beamform_work_dev(None, 1, None, None, None) == -1
    assert L.mi355_beamform_route(None) == b"" and L.mi355_beamform_destroy(None) == 0


def test_python_class_refuses_before_a_context_exists(pkg):
    with pytest.raises(pkg.Mi355Error):
        pkg.clBeamformer(1, 2, 0, 99, 0, 1, 4, 8, 2, 2)  # integration 2 in VOLTAGE mode; device 99 is never looked for
    with pytest.raises(ValueError):
        pkg.clBeamformer(1, 2, 0, 99, 0, 1, 4, 8, 2, 1, False, np.zeros(5, np.int8))
    with pytest.raises(TypeError):
        pkg.clBeamformer(1, 2, 0, 99, 0, 1, 4, 8, 2, 1, False, np.zeros(2 * 8 * 2 * 4, np.float32))


def test_ref_unit_weight_reproduces_a_station():
    rng = np.random.default_rng(3)
    T, S, F, npol, B = 9, 7, 5, 2, 4
    x = ref.frames(rng, T, S, F, npol)
    w = np.zeros((F, npol, B, S, 2), np.int8)
    k, b = 5, 2
    w[:, :, b, k, 0] = 1
    y = ref.voltage(x, w)
    want = x[:, k, :, :, 0].astype(np.float32) + 1j * x[:, k, :, :, 1].astype(np.float32)
    assert np.array_equal(y[:, b], want) and not y[:, [0, 1, 3]].any()
    # j times a station: (re, im) -> (-im, re)
    w[:, :, b, k] = (0, 1)
    assert np.array_equal(ref.voltage(x, w)[:, b], 1j * want)
    p = ref.power_int(x, w, 3)
    assert p.shape == (3, B, F, npol)
    xi = x[:, k].astype(np.int64)
    assert np.array_equal(p[:, b], (xi ** 2).sum(axis=-1).reshape(3, 3, F, npol).sum(axis=1))
    assert np.array_equal(ref.power_int(x, w, 3, True), p.sum(axis=-1))


def test_ref_steers_a_plane_wave():
    """conjugate-phase weights on a synthetic plane wave: S * amplitude on the steered beam (up to the int8 rounding of both)"""
    S, F, npol, B, T = 16, 3, 1, 4, 5
    amp, wamp = 100.0, 100.0
    s = np.arange(S)
    x = np.empty((T, S, F, npol, 2), np.int8)
    w = np.zeros((F, npol, B, S, 2), np.int8)
    phases = [2 * np.pi * s * k / S for k in range(B)]  # beam k looks at a wave with k turns across the array
    wave = np.exp(1j * phases[1])
    for t in range(T):
        v = amp * wave * np.exp(1j * 0.3 * t)
        x[t, :, :, 0, 0] = np.rint(v.real)[:, None]
        x[t, :, :, 0, 1] = np.rint(v.imag)[:, None]
    for k in range(B):
        c = wamp * np.exp(-1j * phases[k])
        w[:, 0, k, :, 0] = np.rint(c.real)
        w[:, 0, k, :, 1] = np.rint(c.imag)
    y = ref.voltage(x, w)
    assert np.all(np.abs(np.abs(y[:, 1]) - S * amp * wamp) <= 2 * S * (amp + wamp))      # rounding: at most ~0.71 per factor and station
    assert np.all(np.abs(y[:, [0, 2, 3]]) <= 2 * S * (amp + wamp))                       # orthogonal beams see only the rounding


def test_ref_asserts_its_bounds():
    x, w = ref.extremes(1, 512, 1, 1, 1)
    re, im = ref.voltage_int(x, w)
    assert int(re.max()) == 16646144 and not im.any()
    x2 = np.concatenate([x, x], axis=1)  # 1024 stations: a component reaches 2^24
    w2 = np.concatenate([w, w], axis=3)
    with pytest.raises(AssertionError):
        ref.voltage_int(x2, w2)
    bad = w.copy()
    bad[0, 0, 0, 0, 0] = -128
    with pytest.raises(AssertionError):
        ref.voltage_int(x, bad)
