"""clFEngine without a device: the sizes of mi355_fengine_plan, every argument error of the contract from _plan / _create with a NULL
context (which shows that the arguments are checked before the context is touched), and the yardstick tests/fengine_ref.py against
hand-computed cases.  The kernels are tested in tests/test_fengine_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import fengine_ref as ref


def _plan(L, S, npol, F, P, shift, n):
    fb, hi, ni = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    rc = L.mi355_fengine_plan(S, npol, F, P, shift, n, C.byref(fb), C.byref(hi), C.byref(ni))
    return rc, (fb.value, hi.value, ni.value), L.mi355_last_error().decode()


def _create(L, S, npol, F, P, shift, ctx=None):
    h = C.c_void_p(1)
    rc = L.mi355_fengine_create(ctx, S, npol, F, P, None, shift, None, C.byref(h))
    assert rc != 0 and not h.value  # no handle comes back from a refused create
    return rc, L.mi355_last_error().decode()


def test_plan_sizes(pkg):
    L = pkg.lib()
    for S, npol, F, P in ((3, 1, 16, 1), (2, 2, 64, 1), (1, 2, 4096, 8), (5, 2, 256, 4), (2, 2, 48, 3), (3, 1, 1000, 2), (64, 2, 1024, 17)):
        for n in (0, 1, 7, 1 << 20):
            want = (2 * S * F * npol, (P - 1) * F, 0 if n == 0 else (n + P - 1) * F)
            assert _plan(L, S, npol, F, P, 0, n)[:2] == (0, want)
            if F % 2 == 0:
                assert _plan(L, S, npol, F, P, 1, n)[:2] == (0, want)
    assert _plan(L, 64, 2, 1024, 4, 1, 100)[1] == (262144, 3072, 103 * 1024)
    assert L.mi355_fengine_plan(4, 1, 16, 1, 0, 5, None, None, None) == 0  # any output pointer may be NULL


BAD = [
    # (S, npol, F, P, shift), message
    ((4, 0, 16, 1, 0), "npol must be 1 or 2"),
    ((4, 3, 16, 1, 0), "npol must be 1 or 2"),
    ((0, 1, 16, 1, 0), "num_inputs must be 1 .. 4096"),
    ((4097, 1, 16, 1, 0), "num_inputs must be 1 .. 4096"),
    ((4, 1, 1, 1, 0), "num_channels must be >= 2"),
    ((4, 1, 0, 1, 0), "num_channels must be >= 2"),
    ((4, 1, -16, 1, 0), "num_channels must be >= 2"),
    ((4, 1, 16, 0, 0), "taps_per_channel must be 1 .. 1024"),
    ((4, 1, 16, 1025, 0), "taps_per_channel must be 1 .. 1024"),
    ((4, 1, 16, 1, 2), "shift must be 0 or 1"),
    ((4, 1, 16, 1, -1), "shift must be 0 or 1"),
    ((4, 1, 15, 1, 1), "shift needs an even num_channels"),
    ((4, 2, 1001, 3, 1), "shift needs an even num_channels"),
]


@pytest.mark.parametrize("args,msg", BAD)
def test_argument_errors_come_before_the_context(pkg, args, msg):
    L = pkg.lib()
    rc, sizes, err = _plan(L, *args, 4)
    assert (rc, sizes, err) == (-1, (0, 0, 0), "invalid argument: " + msg)
    assert _create(L, *args) == (-1, "invalid argument: " + msg)                       # NULL context
    assert _create(L, *args, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: " + msg)  # an invalid one is never touched


def test_create_then_the_context_and_unsupported_sizes(pkg):
    L = pkg.lib()
    assert _create(L, 4, 2, 64, 4, 1) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert _create(L, 3, 1, 1000, 2, 0) == (-1, "invalid argument: NULL context")
    assert L.mi355_fengine_create(None, 4, 2, 64, 4, None, 1, None, None) == -1
    assert _plan(L, 4, 1, 16, 1, 0, -1)[0] == -1
    # a length clFFT refuses, a gain table and a tap table above 1 GiB, an item count past 2^62
    assert _plan(L, 1, 1, (1 << 24) + 2, 1, 0, 1)[0] == -3 and _create(L, 1, 1, (1 << 24) + 2, 1, 0)[0] == -3
    assert _plan(L, 4096, 2, 1 << 16, 1, 0, 1)[0] == -3 and _create(L, 4096, 2, 1 << 16, 1, 0)[0] == -3
    assert _plan(L, 1, 1, 1 << 20, 1024, 0, 1)[0] == -3
    assert _plan(L, 1, 1, 4096, 1, 0, 1 << 61)[0] == -3


def test_null_handles(pkg):
    L = pkg.lib()
    assert L.mi355_fengine_set_gains(None, None) == -1 and L.mi355_fengine_set_input_gain(None, 0, None) == -1
    assert L.mi355_fengine_get_gains(None, None, 0) == -1 and L.mi355_fengine_get_clips(None, None, 0) == -1
    assert L.mi355_fengine_set_generic(None, 1) == -1
    assert L.mi355_fengine_frame_bytes(None) == -1 and L.mi355_fengine_history_items(None) == -1
    assert L.mi355_fengine_work(None, 1, None, None) == -1 and L.mi355_fengine_work_dev(None, 1, None, None, None) == -1
    assert L.mi355_fengine_route(None) == b"" and L.mi355_fengine_destroy(None) == 0


def test_python_class_refuses_before_a_context_exists(pkg):
    with pytest.raises(pkg.Mi355Error):
        pkg.clFEngine(1, 2, 0, 99, 2, 4, 15, None, 1, True)  # shift with an odd length; device 99 is never looked for
    with pytest.raises(ValueError):
        pkg.clFEngine(1, 2, 0, 99, 2, 4, 16, np.ones(17, np.float32), 1)
    with pytest.raises(ValueError):
        pkg.clFEngine(1, 2, 0, 99, 2, 4, 16, None, 1, False, np.ones(5, np.float32))


def test_ref_constants_land_in_channel_zero():
    S, npol, F, T = 3, 2, 16, 5
    c = [complex(3 + r, -(2 + r)) for r in range(S * npol)]
    xs = [np.full(T * F, v, np.complex64) for v in c]
    g = np.full((S * npol, F), 1.0 / F, np.float32)
    for shift in (0, 1):
        res = ref.fengine(xs, None, g, S, npol, F, 1, shift, T)
        want = np.zeros((T, S, F, npol, 2), np.int8)
        for r, v in enumerate(c):
            want[:, r // npol, F // 2 if shift else 0, r % npol] = (v.real, v.imag)
        assert np.array_equal(res.out, want) and not res.clip.any()
        assert res.d.min() > 0.4999  # integers: as far from a boundary as a value gets


def test_ref_arms_by_hand():
    """F = 2, P = 2: z[n] = h[n] x[t F + n] + h[2 + n] x[(t + 1) F + n], X[0] = z0 + z1, X[1] = z0 - z1"""
    x = np.array([1 + 1j, 2, 3j, -1, 5, 1 - 2j], np.complex64)
    h = np.array([1, 2, -1, 0.5], np.float32)
    res = ref.fengine([x], h, None, 1, 1, 2, 2, 0, 2)
    z = [[1 * (1 + 1j) - 1 * 3j, 2 * 2 + 0.5 * -1], [1 * 3j - 1 * 5, 2 * -1 + 0.5 * (1 - 2j)]]
    for t in range(2):
        X = (z[t][0] + z[t][1], z[t][0] - z[t][1])
        for f in range(2):
            assert tuple(res.out[t, 0, f, 0]) == (int(np.rint(X[f].real)), int(np.rint(X[f].imag)))
    # the middle frame is shared: the second call of a split stream starts F items later
    again = ref.fengine([x[2:]], h, None, 1, 1, 2, 2, 0, 1)
    assert np.array_equal(again.out[0], res.out[1])


def test_ref_quantiser_and_distance():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 126.5, 127.49, 127.5, 127.51, -127.5, -128.4, 300.0, np.nan, np.inf, 0.25, -3.75])
    q, clip = ref.quantise(v)
    assert list(q) == [0, 2, 2, 0, -2, 126, 127, 127, 127, -127, -127, 127, 0, 127, 0, -4]       # half to even, symmetric, NaN -> 0
    assert list(clip) == [False] * 7 + [True, True, True, True, True, True, True, False, False]  # rint(127.5) = 128: a clip
    d = ref.distance(v)
    assert np.allclose(d[:6], 0) and np.isclose(d[6], 0.01) and d[7] == 0 and np.isclose(d[8], 0.01) and np.isclose(d[10], 0.9)
    assert d[11] == 172.5 and d[12] == np.inf and d[13] == np.inf and d[14] == 0.25 and d[15] == 0.25
    assert ref.distance(np.array([127.2]))[0] == pytest.approx(0.3) and ref.distance(np.array([127.0]))[0] == 0.5


def test_ref_meets_the_issue_share_at_its_shapes():
    """Gaussian input, gains for an rms of 30 per component: delta stays below 2e-3 and exempts well under 1 % -- from the reference alone"""
    rng = np.random.default_rng(11)
    for S, npol, F, P, T in ((3, 1, 16, 1, 40), (5, 2, 256, 4, 6), (1, 2, 4096, 8, 2)):
        R = S * npol
        h = ref.sinc_taps(F, P)
        xs = [(rng.standard_normal((T + P - 1) * F) + 1j * rng.standard_normal((T + P - 1) * F)).astype(np.complex64) for _ in range(R)]
        X, _ = ref.spectra(xs, h, F, P, T)
        g = (30.0 / np.sqrt((np.abs(X) ** 2).mean(axis=(1, 2)) / 2))[:, None] * np.ones((R, F))
        res = ref.fengine(xs, h, g.astype(np.float32), S, npol, F, P, 1, T)
        assert res.delta.max() < 2e-3
        assert (~res.decided()).mean() < 0.01
        assert 25 < res.out.astype(np.float64).std() < 35
