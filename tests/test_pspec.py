"""CPU: the soundness of clPowerSpectrum's yardstick (tests/pspec_ref.py: against scipy.signal.welch, Parseval, a closed form,
numpy's fftshift), the bookkeeping that needs no device (mi355_pspec_plan), the argument validation and the export."""
import ctypes as C

import numpy as np
import pytest

import pspec_ref as ref

INVALID, UNSUPPORTED = -1, -3


def _plan(L_, N, K, H, S):
    nin, nout = C.c_longlong(-1), C.c_longlong(-1)
    rc = L_.mi355_pspec_plan(N, K, H, S, C.byref(nin), C.byref(nout))
    return rc, (nin.value, nout.value)


@pytest.mark.parametrize("N,K,H", [(64, 5, 64), (64, 7, 32), (100, 4, 37), (256, 3, 1), (17, 6, 17)])
def test_yardstick_against_scipy_welch(N, K, H):
    from scipy import signal
    rng = np.random.default_rng(N + K)
    w = rng.uniform(0.1, 1.0, N).astype(np.float32)
    for win in (w, ref.hann(N)):
        x = ref.make_input(ref.plan(N, K, H, 1)[0], seed=N)
        _, want = signal.welch(x.astype(np.complex128), window=win.astype(np.float64), noverlap=N - H, nfft=N, detrend=False,
                               return_onesided=False, scaling="spectrum", average="mean")
        got = ref.pspec64(x, N, K, H, 1, win, scale=1.0 / float(win.astype(np.float64).sum()) ** 2)[0]
        assert want.shape == got.shape
        assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max())


@pytest.mark.parametrize("N,K,H,S", [(64, 3, 64, 2), (48, 5, 11, 3), (16, 2, 40, 2)])
def test_yardstick_parseval(N, K, H, S):
    w = ref.hann(N)
    x = ref.make_input(ref.plan(N, K, H, S)[0], seed=1)
    P = ref.pspec64(x, N, K, H, S, w)
    f = ref.frames(x, N, K, H, S).astype(np.complex128) * w.astype(np.float64)
    want = N * (np.abs(f) ** 2).sum(axis=2).mean(axis=1)
    assert np.allclose(P.sum(axis=1), want, rtol=1e-12, atol=0)


def test_yardstick_closed_form_tone():
    N, K, b, A = 128, 4, 37, 0.75 - 0.5j
    x = (A * np.exp(2j * np.pi * b * np.arange(K * N) / N))
    P = ref.pspec64(x, N, K, N, 1)[0]
    assert abs(P[b] - N * N * abs(A) ** 2) <= 1e-12 * P[b]
    others = np.delete(P, b)
    assert float(others.max()) <= 1e-20 * P[b]


@pytest.mark.parametrize("N", [8, 9, 64, 101])
def test_yardstick_shift_is_numpys_fftshift(N):
    x = ref.make_input(ref.plan(N, 3, N, 2)[0], seed=N)
    plain, shifted = ref.pspec(x, N, 3, N, 2), ref.pspec(x, N, 3, N, 2, shift=True)
    assert np.array_equal(shifted, np.fft.fftshift(plain, axes=1))
    # clFFT's rule (include/mi355_clenabled.h): out[i] = P[(i + ceil(N / 2)) mod N]
    assert np.array_equal(shifted, plain[:, (np.arange(N) + (N + 1) // 2) % N])


def test_yardstick_db_of_zero_is_minus_inf():
    P = ref.pspec(np.zeros(64, np.complex64), 16, 4, 16, 1, log_output=True)
    assert np.all(np.isneginf(P))


def test_plan_equals_the_yardstick(pkg):
    L_ = pkg.lib()
    for N in (2, 3, 16, 100, 4096, 4099, 32768):
        for K in (1, 2, 7, 1000):
            for H in sorted({1, 3, max(N // 2, 1), N, N + 5, 3 * N}):
                for S in (0, 1, 2, 17, 1 << 40):
                    rc, got = _plan(L_, N, K, H, S)
                    want = ref.plan(N, K, H, S)
                    if max(want) > 1 << 62:  # (a long long holds no more: the contract's own limit)
                        assert rc == UNSUPPORTED and got == (0, 0), (N, K, H, S, got)
                    else:
                        assert rc == 0 and got == want, (N, K, H, S, got)
    rc, got = _plan(L_, 4096, 64, 2048, 1 << 40)
    assert rc == 0 and got == (((1 << 46) - 1) * 2048 + 4096, 1 << 52)
    assert L_.mi355_pspec_plan(64, 4, 64, 10, None, None) == 0  # NULL outputs are allowed


def test_validation(pkg):
    L_ = pkg.lib()
    for N, K, H, S in ((0, 1, 1, 1), (-4, 1, 1, 1), (64, 0, 64, 1), (64, -1, 64, 1), (64, 4, 0, 1), (64, 4, -2, 1), (64, 4, 64, -1)):
        assert _plan(L_, N, K, H, S)[0] == INVALID, (N, K, H, S)
    # what mi355_fft_create refuses: clFFT's own words
    for N in (1, 16777216 * 2, 8388609):
        assert _plan(L_, N, 4, N, 1)[0] == UNSUPPORTED
        msg = L_.mi355_last_error()
        assert b"fft size %d unsupported" % N in msg and b"powers of two 2..16777216" in msg, msg
    assert _plan(L_, 16777216, 1, 1, 1)[0] == 0 and _plan(L_, 8388607, 1, 1, 1)[0] == 0
    # counts past 2^62
    assert _plan(L_, 4096, 1 << 20, 1 << 20, 1 << 40)[0] == UNSUPPORTED and b"2^62" in L_.mi355_last_error()
    # create refuses what it can tell without a device before it looks at the context
    h = C.c_void_p()
    w = np.ones(64, np.float32)
    wp = w.ctypes.data_as(C.c_void_p)

    def create(N, K, H, win=None, wlen=0, ctx=None):
        return L_.mi355_pspec_create(ctx, N, win, wlen, K, H, 0, 0, 1.0, C.byref(h))

    for args in ((0, 4, 64), (64, 0, 64), (64, 4, 0), (-1, 4, 64)):
        assert create(*args) == INVALID and not h.value, args
    assert create(64, 4, 64, wp, 63) == INVALID and b"window" in L_.mi355_last_error()
    assert create(64, 4, 64, wp, 65) == INVALID
    assert create(64, 4, 64, None, 64) == INVALID and b"window is NULL" in L_.mi355_last_error()
    assert create(1, 4, 1) == UNSUPPORTED and b"fft size 1 unsupported" in L_.mi355_last_error()
    assert create(1 << 25, 4, 64) == UNSUPPORTED
    assert create(64, 4, 32, wp, 64) == INVALID and b"NULL argument" in L_.mi355_last_error()  # all fine but the context
    assert not h.value
    # NULL handles
    assert L_.mi355_pspec_destroy(None) == 0
    for fn in ("fft_size", "navg", "hop"):
        assert getattr(L_, "mi355_pspec_" + fn)(None) == INVALID
    assert L_.mi355_pspec_route(None) == b""
    assert L_.mi355_pspec_work(None, 1, None, None) == INVALID and L_.mi355_pspec_work_dev(None, 1, None, None, None) == INVALID
    assert L_.mi355_pspec_set_scale(None, 1.0) == INVALID and L_.mi355_pspec_set_window(None, wp, 64) == INVALID
    assert L_.mi355_pspec_set_generic(None, 1) == INVALID


def test_python_class_is_exported(pkg):
    assert pkg.clenabled.clPowerSpectrum is pkg.clPowerSpectrum
    for name in ("plan", "history", "route", "set_scale", "set_window", "set_generic", "work", "general_work", "work_device", "stop"):
        assert callable(getattr(pkg.clPowerSpectrum, name))
