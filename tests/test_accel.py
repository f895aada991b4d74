"""clAccelResampler without a device: the index map's properties with Python integers, the library's host helpers against them, and
every refusal that needs no device.  The kernels run on the GPU in tests/test_accel_gpu.py, the C++ block in tests/test_accel_host.py."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest

import accel_ref as ref

SIZES = [256, 4099, 8192, 1 << 22]


def _coeffs(N):
    rng = np.random.default_rng(N)
    top = ref.cmax(N)
    return [0, 1, -1, top, -top] + [int(v) for v in rng.integers(-top, top, 3, dtype=np.int64)] + [ref.apex(N), -ref.apex(N, 3)]


@functools.lru_cache(maxsize=None)
def _src(N, c):
    s = ref.src_array(N, c)
    s.setflags(write=False)
    return s


def test_the_vectorised_yardstick_is_the_integer_one():
    """src_array (32-bit limbs) against src (Python integers): whole rows at the small sizes, windows at N = 2^22"""
    for N in SIZES[:3]:
        for c in _coeffs(N):
            assert _src(N, c).tolist() == ref.src(N, c), (N, c)
    N = SIZES[3]
    for c in _coeffs(N):
        for i0 in (0, 1 << 20, (1 << 21) - 300, (1 << 22) - 600, 1234567):
            assert _src(N, c)[i0:i0 + 600].tolist() == ref.src(N, c, i0, 600), (c, i0)


@pytest.mark.parametrize("N", SIZES)
def test_properties_of_the_map(N):
    """end points, monotonicity and |delta| <= N / 8 at c = 0, +-1, +-2^63 / N, random values and two apex coefficients"""
    i = np.arange(N, dtype=np.int64)
    assert ref.cmax(N) * N <= 1 << 63 < (ref.cmax(N) + 1) * N
    for c in _coeffs(N):
        s = _src(N, c)
        assert s[0] == 0 and s[-1] == N - 1, c
        assert (np.diff(s) >= 0).all(), c
        assert 8 * np.abs(s - i).max() <= N, c
        if c == 0:
            assert np.array_equal(s, i)
    # the bound is reached: at c = +-2^63 / N the largest shift is N / 8 (rounded to nearest for the odd N)
    for sign in (1, -1):
        shift = sign * (_src(N, sign * ref.cmax(N)) - i)
        assert shift.min() == 0 and shift.max() == (N * N // 4 * ref.cmax(N) + (1 << 63)) >> 64
    if N % 8 == 0:
        assert (_src(N, ref.cmax(N)) - i).max() == N // 8
    # monotone in c as well: the tiled route's window is [src_cmin(i0), src_cmax(i1)]
    cs = sorted(_coeffs(N))
    for lo, hi in zip(cs, cs[1:]):
        assert (_src(N, lo) <= _src(N, hi)).all()


def test_issue_figures():
    """c = +-2^63 / N at N = 2^14: monotone, end points fixed, the largest shift exactly N / 8"""
    N = 1 << 14
    for sign in (1, -1):
        s = ref.src(N, sign * ref.cmax(N))
        assert s[0] == 0 and s[-1] == N - 1 and all(b >= a for a, b in zip(s, s[1:]))
        assert max(sign * (v - i) for i, v in enumerate(s)) == N // 8


@pytest.mark.parametrize("N", SIZES[:3])
def test_index_helper_whole_rows(pkg, N):
    for c in _coeffs(N):
        assert np.array_equal(pkg.accel_index(N, c), _src(N, c)), c


def test_index_helper_windows(pkg):
    for N in SIZES:
        for c in _coeffs(N)[3:]:
            for i0, count in ((0, 1), (N - 1, 1), (N // 2 - 7, 15), (N - 200, 200), (17, 0), (N, 0)):
                assert pkg.accel_index(N, c, i0, count).tolist() == ref.src(N, c, i0, count), (N, c, i0, count)
    N = 1 << 22
    assert np.array_equal(pkg.accel_index(N, -ref.cmax(N)), _src(N, -ref.cmax(N)))
    L = pkg.lib()
    buf = np.zeros(4, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    for n, c, i0, count in ((255, 0, 0, 1), ((1 << 22) + 1, 0, 0, 1), (256, ref.cmax(256) + 1, 0, 1), (256, -ref.cmax(256) - 1, 0, 1),
                            (256, 0, -1, 1), (256, 0, 0, -1), (256, 0, 254, 3), (256, 0, 257, 0)):
        assert L.mi355_accel_index(n, c, i0, count, p) == -1, (n, c, i0, count)
    assert L.mi355_accel_index(256, 0, 0, 1, None) == -1


def test_truncation_toward_zero_is_another_function():
    N = 8192
    c = -ref.cmax(N)
    differ = sum(a != b for a, b in zip(ref.src(N, c), ref.src_truncating(N, c)))
    print("N = %d, c = -2^63 / N: truncation toward zero changes %d of %d indices" % (N, differ, N))
    assert differ > 0
    assert ref.src(N, -c) == ref.src_truncating(N, -c)  # (a non-negative product: the two agree)


def test_coeff_within_two_units_of_the_rational_value(pkg):
    rng = np.random.default_rng(5)
    cases = [(1 << 20, 64e-6, 0.0), (1 << 20, 64e-6, 250.0), (1 << 20, 64e-6, -250.0), (256, 1e-3, 1e5), (1 << 22, 81.92e-6, 3.3),
             (4099, 0.1, -7.25), (1 << 14, 1e-9, 1e-9), (1 << 14, 5e-324, 1.0)]
    cases += [(int(n), float(t), float(a)) for n, t, a in zip(rng.integers(256, 1 << 22, 40), 10.0 ** rng.uniform(-6, -2, 40),
                                                                rng.uniform(-500, 500, 40))]
    checked = 0
    for n, tsamp, acc in cases:
        exact = ref.coeff_exact(tsamp, acc)
        if abs(exact) * n > (1 << 63) - 2 * n:
            continue
        c = pkg.accel_coeff(n, tsamp, acc)
        assert abs(Fraction(c) - exact) <= 2, (n, tsamp, acc, c, float(exact))
        checked += 1
    assert checked >= 40
    assert pkg.accel_coeff(1 << 20, 64e-6, 0.0) == 0 and pkg.accel_coeff(1 << 20, 64e-6, 100.0) < 0 < pkg.accel_coeff(1 << 20, 64e-6, -100.0)


def test_coeff_refusals(pkg):
    L = pkg.lib()
    c = C.c_longlong(77)
    N, tsamp = 1 << 20, 64e-6
    edge = float(Fraction(1 << 63, N) * 2 * ref.LIGHT / (Fraction(tsamp) * (1 << 64)))   # |accel| at which |c| N = 2^63
    assert L.mi355_accel_coeff(N, tsamp, 0.999 * edge, C.byref(c)) == 0 and abs(c.value) * N <= 1 << 63
    for n, t, a in ((N, tsamp, 1.001 * edge), (N, tsamp, -1.001 * edge), (N, tsamp, 1e300), (N, tsamp, float("inf")), (N, tsamp, float("nan")),
                    (N, 0.0, 1.0), (N, -1e-3, 1.0), (N, float("inf"), 1.0), (N, float("nan"), 1.0), (255, tsamp, 1.0), ((1 << 22) + 1, tsamp, 1.0)):
        c.value = 77
        assert L.mi355_accel_coeff(n, t, a, C.byref(c)) == -1 and c.value == 0, (n, t, a)
    assert L.mi355_accel_coeff(N, tsamp, 1.0, None) == -1
    with pytest.raises(pkg.Mi355Error):
        pkg.accel_coeff(N, tsamp, 1.001 * edge)


def test_trial_ladder(pkg):
    N, tsamp = 1 << 20, 64e-6
    for a_lo, a_hi, tol in ((-500.0, 500.0, 1.0), (-500.0, 500.0, 2.5), (10.0, 700.0, 1.0), (-3.0, 2.0, 0.25), (-40.0, -39.0, 1.0)):
        da = Fraction(tol) * 8 * ref.LIGHT / (Fraction(tsamp) * N * N)
        js = [j for j in range(int(Fraction(a_lo) / da) - 2, int(Fraction(a_hi) / da) + 3) if a_lo <= j * da <= a_hi]
        c, count = pkg.accel_trials(N, tsamp, a_lo, a_hi, tol)
        assert count == len(js) == len(c), (a_lo, a_hi, tol)
        # the ladder covers [a_lo, a_hi]: the first and the last trial lie less than one step inside the ends
        if js:
            assert js[0] * da - Fraction(a_lo) < da and Fraction(a_hi) - js[-1] * da < da
        else:
            assert Fraction(a_hi) - Fraction(a_lo) < da
        for j, cj in zip(js, c.tolist()):
            assert abs(Fraction(cj) - ref.coeff_exact(tsamp, 1.0) * j * da) <= 2, j   # the coefficient of a_j = j da
            if j == 0:
                assert cj == 0
        assert (0 in js) == (0 in c.tolist())
        # neighbours differ by tol samples at mid-observation, within one sample of rounding
        mid = [ref.delta(N, int(cj), N // 2) for cj in c.tolist()]
        assert all(abs(b - a) <= tol + 1 for a, b in zip(mid, mid[1:]))
        if tol >= 1 and len(mid) > 1:
            assert all(a != b for a, b in zip(mid, mid[1:]))
    # count is the whole ladder, cap limits what is stored
    c_all, count = pkg.accel_trials(N, tsamp, -500.0, 500.0, 1.0)
    c_cap, count_cap = pkg.accel_trials(N, tsamp, -500.0, 500.0, 1.0, cap=5)
    assert count_cap == count > 5 and len(c_cap) == 5 and np.array_equal(c_cap, c_all[:5])
    cnt = C.c_longlong(-1)
    L = pkg.lib()
    assert L.mi355_accel_trials(N, tsamp, -500.0, 500.0, 1.0, None, 0, C.byref(cnt)) == 0 and cnt.value == count
    for args in ((N, tsamp, 1.0, -1.0, 1.0), (N, tsamp, 0.0, 1.0, 0.0), (N, tsamp, 0.0, 1.0, -1.0), (N, 0.0, 0.0, 1.0, 1.0),
                 (255, tsamp, 0.0, 1.0, 1.0), (N, tsamp, float("nan"), 1.0, 1.0), (N, tsamp, 0.0, float("inf"), 1.0),
                 (N, tsamp, -1e9, 1e9, 1.0)):   # the last: trials outside |c| N <= 2^63
        assert L.mi355_accel_trials(*args, None, 0, C.byref(cnt)) == -1 and cnt.value == 0, args
    assert L.mi355_accel_trials(N, tsamp, 0.0, 1.0, 1.0, None, 3, C.byref(cnt)) == -1
    assert L.mi355_accel_trials(N, tsamp, 0.0, 1.0, 1.0, None, 0, None) == -1


def test_plan_and_create_refuse_before_any_device_is_looked_for(pkg):
    L = pkg.lib()
    assert pkg.clAccelResampler.plan(3, 4099, 8) == (24, ref.TILE, 64)
    assert pkg.clAccelResampler.plan(1 << 20, 256, 4096)[0] == 1 << 32
    r = C.c_longlong(5)
    for S, N, A in ((0, 256, 1), ((1 << 20) + 1, 256, 1), (1, 255, 1), (1, (1 << 22) + 1, 1), (1, 256, 0), (1, 256, 4097), (-1, 256, 1)):
        assert L.mi355_accel_plan(S, N, A, C.byref(r), None, None) == -1 and r.value == 0, (S, N, A)
        h = C.c_void_p(1)
        assert L.mi355_accel_create(None, S, N, A, None, C.byref(h)) == -1 and not h.value
    # 2^20 series of 2^22 words: more than 2^40 bytes
    assert L.mi355_accel_plan(1 << 20, 1 << 22, 1, None, None, None) == -3
    # a coefficient outside the bound, before the (missing) context is looked at
    h = C.c_void_p(1)
    bad = np.array([0, ref.cmax(256) + 1], np.int64)
    assert L.mi355_accel_create(None, 1, 256, 2, C.c_void_p(bad.ctypes.data), C.byref(h)) == -1 and not h.value
    assert b"|c| n" in L.mi355_last_error()
    ok = np.array([0, ref.cmax(256)], np.int64)
    assert L.mi355_accel_create(None, 1, 256, 2, C.c_void_p(ok.ctypes.data), C.byref(h)) == -1 and b"NULL context" in L.mi355_last_error()
    assert L.mi355_accel_create(None, 1, 256, 2, None, None) == -1
    for fn in (L.mi355_accel_set_trials, L.mi355_accel_set_generic):
        assert fn(None, None if fn is L.mi355_accel_set_trials else 1) == -1
    assert L.mi355_accel_route(None) == b"" and L.mi355_accel_destroy(None) == 0
    with pytest.raises(pkg.Mi355Error):
        pkg.clAccelResampler(1, 2, 0, 0, 3, 100, [0])   # refused by plan(), before a context exists


def test_plan_of_the_tiled_route():
    """the yardstick's copy of the group plan: one trial always fits, a ladder at one sample per step takes 16, a widely spread table 1;
    the window bound holds at every tile"""
    assert ref.ONE_TRIAL < ref.LDS_WORDS
    for N in (256, 4099, 8192, 1 << 20):
        top = ref.cmax(N)
        step = -((-(1 << 66)) // (N * N))      # one sample at mid-observation
        ladder = [j * step for j in range(-20, 21)]
        assert ref.group(N, ladder) == 16
        assert ref.group(N, [0, top, -top, 5]) == (1 if N > 8192 else ref.group(N, [0, top, -top, 5]))
        for trials in ([top], [-top], ladder[:16], ladder[-16:], [0, top, -top, 5]):
            g = ref.group(N, trials)
            for a in range(0, len(trials), g):
                for i0 in range(0, N, ref.TILE):
                    part = trials[a:a + g]
                    bound = ref.ONE_TRIAL - 3 + -((-(max(part) - min(part)) * N * N) >> 66)
                    assert ref.window_words(N, part, i0) <= bound <= ref.LDS_WORDS - 3, (N, part, i0)
    assert ref.group(1 << 20, [0, ref.cmax(1 << 20), -ref.cmax(1 << 20), 5]) == 1
