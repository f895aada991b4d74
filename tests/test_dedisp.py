"""clDedisperser without a device: the sizes of mi355_dedisp_plan, every argument error of the contract from _plan / _create with a NULL
context (which shows that the arguments and the table are checked before the context is touched), NULL handles, the self-checks of the
yardstick tests/dedisp_ref.py, and the host-only delay helper mi355_dedisp_delays against its numpy restatement.  The kernels are tested
in tests/test_dedisp_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import dedisp_ref as ref


def _plan(L, R, F, D, H, order):
    fi, hi, fo = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    rc = L.mi355_dedisp_plan(R, F, D, H, order, C.byref(fi), C.byref(hi), C.byref(fo))
    return rc, (fi.value, hi.value, fo.value), L.mi355_last_error().decode()


def _create(L, R, F, D, H, order, tab=None, ctx=None):
    h = C.c_void_p(1)
    tp = None if tab is None else C.c_void_p(tab.ctypes.data)
    rc = L.mi355_dedisp_create(ctx, R, F, D, H, order, tp, C.byref(h))
    assert rc != 0 and not h.value  # no handle comes back from a refused create
    return rc, L.mi355_last_error().decode()


def test_plan_sizes(pkg):
    L = pkg.lib()
    for R, F, D, H in ((64, 1024, 1024, 1000), (1, 1, 1, 0), (3, 80, 40, 200), (4096, 16384, 4096, 1 << 20)):
        for order in (ref.TRIAL_MAJOR, ref.TIME_MAJOR):
            assert _plan(L, R, F, D, H, order)[:2] == (0, ref.plan(R, F, D, H))
    assert _plan(L, 64, 1024, 512, 777, 1)[1] == (65536, 777, 32768)
    assert L.mi355_dedisp_plan(2, 8, 4, 5, 0, None, None, None) == 0  # any output pointer may be NULL


BAD = [
    # (R, F, D, H, order), message
    ((0, 8, 4, 5, 0), "num_rows must be 1 .. 4096"),
    ((4097, 8, 4, 5, 0), "num_rows must be 1 .. 4096"),
    ((2, 0, 4, 5, 0), "num_channels must be 1 .. 16384"),
    ((2, 16385, 4, 5, 0), "num_channels must be 1 .. 16384"),
    ((2, 8, 0, 5, 0), "num_trials must be 1 .. 4096"),
    ((2, 8, 4097, 5, 0), "num_trials must be 1 .. 4096"),
    ((2, 8, 4, -1, 0), "max_delay must be 0 .. 2^20"),
    ((2, 8, 4, (1 << 20) + 1, 0), "max_delay must be 0 .. 2^20"),
    ((2, 8, 4, 5, 2), "order must be TRIAL_MAJOR (0) or TIME_MAJOR (1)"),
    ((2, 8, 4, 5, -1), "order must be TRIAL_MAJOR (0) or TIME_MAJOR (1)"),
]


@pytest.mark.parametrize("args,msg", BAD)
def test_argument_errors_come_before_the_context(pkg, args, msg):
    L = pkg.lib()
    rc, sizes, err = _plan(L, *args)
    assert (rc, sizes, err) == (-1, (0, 0, 0), "invalid argument: " + msg)
    assert _create(L, *args) == (-1, "invalid argument: " + msg)                              # NULL context
    assert _create(L, *args, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: " + msg)  # an invalid one is never touched


def test_create_checks_the_table_then_the_context(pkg):
    L = pkg.lib()
    R, F, D, H = 2, 8, 4, 5
    tab = np.zeros((D, F), np.int32)
    assert _create(L, R, F, D, H, 1, tab) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert _create(L, R, F, D, H, 1, None) == (-1, "invalid argument: NULL context")
    for pos in ((0, 0), (D - 1, F - 1), (2, 3)):
        for v in (-2, H + 1, -(1 << 31), (1 << 31) - 1):
            bad = tab.copy()
            bad[pos] = v
            assert _create(L, R, F, D, H, 1, bad, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: a delay outside -1 .. max_delay")
    ok = tab.copy()
    ok[0, 0], ok[1, 1] = -1, H
    assert _create(L, R, F, D, H, 1, ok) == (-1, "invalid argument: NULL context")
    assert _create(L, R, F, D, 0, 1, np.full((D, F), -1, np.int32)) == (-1, "invalid argument: NULL context")  # H = 0: -1 and 0 are the table
    assert L.mi355_dedisp_create(None, R, F, D, H, 1, None, None) == -1


def test_null_handles(pkg):
    L = pkg.lib()
    assert L.mi355_dedisp_set_delays(None, None) == -1 and L.mi355_dedisp_get_delays(None, None, 0) == -1
    assert L.mi355_dedisp_set_generic(None, 1) == -1 and L.mi355_dedisp_history(None) == -1
    assert L.mi355_dedisp_work(None, 1, None, None, 1) == -1 and L.mi355_dedisp_work_dev(None, 1, None, None, 1, None) == -1
    assert L.mi355_dedisp_route(None) == b"" and L.mi355_dedisp_destroy(None) == 0


def test_python_class_refuses_before_a_context_exists(pkg):
    with pytest.raises(pkg.Mi355Error):
        pkg.clDedisperser(1, 2, 0, 99, 2, 8, 4, -1)  # max_delay; device 99 is never looked for
    with pytest.raises(ValueError):
        pkg.clDedisperser(1, 2, 0, 99, 2, 8, 4, 5, 1, np.zeros(5, np.int32))
    with pytest.raises(TypeError):
        pkg.clDedisperser(1, 2, 0, 99, 2, 8, 4, 5, 1, np.zeros((4, 8), np.float32))


def test_ref_impulse_comes_back_on_its_trial():
    """an impulse dispersed by trial k of a table: F on (trial k, time of the impulse), and F ones in every trial in total"""
    F, D, H, n, t0, k = 24, 6, 30, 40, 7, 4
    tab, top = ref.delays(1500.0, -10.0, F, 1e-3, np.arange(D) * 6.0)
    assert top <= H and top > D  # the trials differ
    x = np.zeros((n + H, 1, F), np.float32)
    for f in range(F):
        x[t0 + tab[k, f], 0, f] = 1.0
    y = ref.dedisperse(x, tab, n, ref.TRIAL_MAJOR)[0]
    assert y[k, t0] == F and np.argmax(y.max(axis=1)) == k and y[k].sum() == F
    for d in range(D):
        assert y[d].sum() == F and (d == k or y[d].max() < F)
    assert np.array_equal(ref.dedisperse(x, tab, n, ref.TIME_MAJOR)[:, 0, :], y.T)


def test_ref_killed_channels_and_order():
    rng = np.random.default_rng(1)
    x = ref.gaussian(rng, 12, 2, 9)
    tab = ref.random_table(rng, 3, 9, 4)
    tab[1, :] = -1
    y = ref.dedisperse(x, tab, 8)
    assert not y[:, :, 1].any() and not np.signbit(y[:, :, 1]).any()  # an all-(-1) trial is +0.0
    x2 = x.copy()
    x2[:, :, 4] = np.nan
    tab2 = tab.copy()
    tab2[:, 4] = -1
    assert np.isfinite(ref.dedisperse(x2, tab2, 8)).all()  # a NaN in a killed channel reaches nothing
    # the order is the contract: the float64 sum rounded once differs from the chain of float32 roundings somewhere
    z = np.zeros((3, 9), np.int32)
    assert not np.array_equal(ref.dedisperse(x, z, 12)[:, :, 0], x.astype(np.float64).sum(axis=2).astype(np.float32))
    with pytest.raises(AssertionError):
        ref.dedisperse(x, tab, 9)  # reads past the input


BANDS = [
    # f0 MHz, df MHz, F, tsamp s, dm list
    (1200.0, 300.0 / 80, 80, 1e-3, np.arange(40) * 2.37 + 0.11),
    (1500.0, -300.0 / 64, 64, 6.4e-5, np.arange(33) * 0.731 + 0.05),
]


@pytest.mark.parametrize("f0,df,F,tsamp,dm", BANDS)
def test_delay_helper_equals_numpy(pkg, f0, df, F, tsamp, dm):
    exact = ref.delays(f0, df, F, tsamp, dm, exact=True)
    frac = np.abs(exact - np.floor(exact) - 0.5)
    assert frac.min() > 1e-9, "a reference value lies on a rounding boundary: choose another dm list"
    want, top = ref.delays(f0, df, F, tsamp, dm)
    got, got_top = pkg.dedisp_delays(f0, df, F, tsamp, dm)
    assert got.dtype == np.int32 and np.array_equal(got, want) and got_top == top == int(want.max())
    ref_col = 0 if df < 0 else F - 1
    assert not want[:, ref_col].any() and top > 50  # the highest channel is the reference; the table is no trivial one
    assert np.all(np.diff(want, axis=0) >= 0)        # more dispersion measure, more delay


def test_delay_helper_refusals(pkg):
    L = pkg.lib()
    out = np.zeros(8, np.int32)
    top = C.c_int(7)

    def call(f0, df, F, ts, dm):
        d = np.asarray(dm, np.float64)
        return L.mi355_dedisp_delays(f0, df, F, ts, C.c_void_p(d.ctypes.data), d.size, C.c_void_p(out.ctypes.data), C.byref(top))

    assert call(1200.0, 10.0, 4, 1e-3, [0.0, 10.0]) == 0 and top.value == int(out.max())
    assert call(1200.0, 10.0, 4, 0.0, [1.0]) == -1 and call(1200.0, 10.0, 4, -1e-3, [1.0]) == -1
    assert call(0.0, 10.0, 4, 1e-3, [1.0]) == -1 and call(20.0, -10.0, 4, 1e-3, [1.0]) == -1      # a channel at or below 0 MHz
    assert call(1200.0, 10.0, 4, 1e-3, [-1.0]) == -1 and call(1200.0, 10.0, 4, 1e-3, [np.nan]) == -1
    assert call(1200.0, 10.0, 4, 1e-3, [np.inf]) == -1
    assert call(100.0, 10.0, 4, 1e-6, [1000.0]) == -1                                                 # a delay above 2^20
    assert call(1200.0, 10.0, 0, 1e-3, [1.0]) == -1
    assert L.mi355_dedisp_delays(1200.0, 10.0, 4, 1e-3, None, 1, C.c_void_p(out.ctypes.data), None) == -1
    assert L.mi355_last_error().decode().startswith("invalid argument")
