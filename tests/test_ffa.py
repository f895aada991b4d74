"""clPeriodSearch without a device: the yardstick tests/ffa_ref.py against the direct sum over rows with shift(L, i, r) on integer-valued
inputs (where every order of summation is exact: this pins the shift pattern independently of the tree), the proof that a
left-to-right row sum is another function than the tree, the library's exports against the header, mi355_ffa_shift / _period / _plan
and every create-time refusal through the C ABI with a NULL context (which shows that the arguments are checked before the context is
touched), and the recorded injected-pulsar case.  The kernels are tested in tests/test_ffa_gpu.py."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import ffa_ref as ref

NAMES = {"plan", "create", "destroy", "set_stats", "get_stats", "set_generic", "route", "work", "work_dev", "shift", "period"}
INVALID, UNSUPPORTED = -1, -3


def _direct(rows, L):
    """y[i][j] = sum over rows r of row r at (j + shift(L, i, r)) mod p, left to right"""
    m, p = rows.shape
    j = np.arange(p)
    y = np.zeros((m, p), np.float32)
    for i in range(m):
        for r in range(m):
            y[i] = y[i] + rows[r][(j + ref.shift(L, i, r)) % p]
    return y


@pytest.mark.parametrize("p", [16, 37])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
def test_tree_equals_the_direct_sum_on_integers(L, p):
    rng = np.random.default_rng(100 * L + p)
    rows = rng.integers(-8, 9, (1 << L, p)).astype(np.float32)
    assert np.array_equal(ref.transform(rows), _direct(rows, L))


def test_a_left_to_right_sum_is_another_function():
    rng = np.random.default_rng(5)
    rows = rng.gamma(2.0, 3.0, (32, 37)).astype(np.float32)
    tree, lr = ref.transform(rows), _direct(rows, 5)
    assert not np.array_equal(tree.view(np.uint32), lr.view(np.uint32))
    assert np.allclose(tree, lr, rtol=1e-5)


@pytest.mark.parametrize("L", [1, 2, 5, 8])
def test_shift_properties(L):
    """sh(i, m - 1) = i and the path stays within 1.5 bins of the straight line"""
    m = 1 << L
    for i in range(m):
        assert ref.shift(L, i, m - 1) == i and ref.shift(L, i, 0) == 0
        for r in range(m):
            assert abs(ref.shift(L, i, r) - Fraction(r * i, m - 1)) < Fraction(3, 2)


def test_header_symbols_are_exported(pkg):
    with open(os.path.join(ROOT, "include", "mi355_clenabled.h")) as f:
        declared = set(re.findall(r"^[a-z][a-z ]*\*?\b(mi355_ffa_\w+)\(", f.read(), re.M))
    assert declared == {"mi355_ffa_" + n for n in NAMES}
    L = pkg.lib()
    for name in sorted(declared):
        assert getattr(L, name) is not None, name
    assert callable(pkg.ffa_shift) and callable(pkg.ffa_period) and pkg.clPeriodSearch.shift is pkg.ffa_shift


def test_shift_and_period_through_the_c_abi(pkg):
    L = pkg.lib()
    for lg in (1, 3, 6, 12):
        m = 1 << lg
        for i in sorted({0, 1, m // 2, m - 1}):
            for r in sorted({0, 1, m // 3, m - 1}):
                assert L.mi355_ffa_shift(lg, i, r) == ref.shift(lg, i, r)
    for bad in [(0, 0, 0), (13, 0, 0), (3, 8, 0), (3, 0, 8), (3, -1, 0), (3, 0, -1)]:
        assert L.mi355_ffa_shift(*bad) == INVALID
        with pytest.raises(ValueError):
            pkg.ffa_shift(*bad)
    assert pkg.ffa_period(37, 5, 11, 1.0) == 37 + 11 / 31
    assert pkg.ffa_period(16, 1, 1, 0.5) == 8.5
    assert pkg.ffa_period(4096, 12, 4095, 64e-6) == 4097 * 64e-6
    for bad in [(15, 5, 0, 1.0), (4097, 5, 0, 1.0), (37, 0, 0, 1.0), (37, 13, 0, 1.0), (37, 5, 32, 1.0), (37, 5, -1, 1.0), (37, 5, 0, 0.0),
                (37, 5, 0, float("nan")), (37, 5, 0, float("inf"))]:
        assert np.isnan(L.mi355_ffa_period(*bad))
        with pytest.raises(ValueError):
            pkg.ffa_period(*bad)


def _plan(L, *shape):
    out = [C.c_longlong(-1) for _ in range(4)]
    rc = L.mi355_ffa_plan(*shape, *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out), L.mi355_last_error().decode()


def test_plan_sizes(pkg):
    L = pkg.lib()
    rc, (N, rec, prof, scratch), _ = _plan(L, 2, 250, 251, 12, 7)
    assert rc == 0 and N == 4096 * 251 and rec == 2 * 4096 and prof == 2 * 4096 * 251
    assert scratch >= 2 * 4 * 2 * N  # two planes of S m p floats at least
    rc, (N, rec, prof, scratch), _ = _plan(L, 1, 16, 16, 1, 1)
    assert rc == 0 and (N, rec, prof) == (32, 2, 32) and scratch >= 2 * 4 * 32
    assert L.mi355_ffa_plan(1, 16, 16, 1, 1, None, None, None, None) == 0
    assert pkg.clPeriodSearch.plan(3, 16, 19, 3, 4)[:3] == (8 * 19, 4 * 8, 4 * 8 * 19)


REFUSED = [
    ((0, 16, 16, 1, 1), INVALID, "num_series"),
    (((1 << 20) + 1, 16, 16, 1, 1), INVALID, "num_series"),
    ((1, 15, 16, 1, 1), INVALID, "base periods"),
    ((1, 17, 16, 1, 1), INVALID, "base periods"),
    ((1, 16, 4097, 1, 1), INVALID, "base periods"),
    ((1, 16, 16, 0, 1), INVALID, "log2_rows"),
    ((1, 16, 16, 13, 1), INVALID, "log2_rows"),
    ((1, 16, 16, 1, 0), INVALID, "num_widths"),
    ((1, 2048, 4096, 1, 12), INVALID, "num_widths"),
    ((1, 16, 32, 3, 6), INVALID, "widest boxcar"),       # 2^5 = 32 > p_lo = 16
    ((1, 31, 32, 3, 6), INVALID, "widest boxcar"),
    ((1 << 20, 4096, 4096, 12, 1), UNSUPPORTED, "2^40"),  # 2^46 bytes of input
    ((1 << 20, 16, 4096, 6, 1), UNSUPPORTED, "2^40"),     # 2^20 x 4081 x 64 records of 8 bytes
]


@pytest.mark.parametrize("shape,code,word", REFUSED)
def test_refusals_without_a_device(pkg, shape, code, word):
    L = pkg.lib()
    rc, sizes, msg = _plan(L, *shape)
    assert rc == code and sizes == (0, 0, 0, 0) and word in msg, msg
    h = C.c_void_p(1)
    rc = L.mi355_ffa_create(None, *shape, None, None, C.byref(h))  # a NULL context: refused for the shape, not for the context
    assert rc == code and not h.value and word in L.mi355_last_error().decode()
    with pytest.raises(pkg.Mi355Error):
        pkg.clPeriodSearch(0, 0, 0, 0, *shape)


def test_limits_are_accepted_and_null_handles_refused(pkg):
    L = pkg.lib()
    assert _plan(L, 1, 1024, 4096, 12, 11)[0] == 0 and _plan(L, 1 << 20, 16, 16, 1, 5)[0] == 0
    h = C.c_void_p(1)
    assert L.mi355_ffa_create(None, 1, 16, 16, 1, 1, None, None, C.byref(h)) == INVALID and not h.value  # now it is the context
    assert "context" in L.mi355_last_error().decode()
    assert L.mi355_ffa_create(None, 1, 16, 16, 1, 1, None, None, None) == INVALID
    assert L.mi355_ffa_destroy(None) == 0 and L.mi355_ffa_route(None) == b""
    assert L.mi355_ffa_set_generic(None, 1) == INVALID and L.mi355_ffa_set_stats(None, None, None) == INVALID
    assert L.mi355_ffa_get_stats(None, None, None, 0) == INVALID
    assert L.mi355_ffa_work(None, None, 0, None, None) == INVALID and L.mi355_ffa_work_dev(None, None, 0, None, None, None) == INVALID


def test_key_order_of_the_yardstick():
    """+0 above -0, the smallest k of equals, then the smallest j; NaN never takes part; nothing but NaN gives {-Inf, 0xFFFFFFFF}"""
    y = np.zeros((2, 16), np.float32)
    y[0, 5] = -0.0
    rec = ref.records(ref.keys(y, 1, 3, 0.0, 1.0))
    assert rec["loc"][0] == 0 and rec["loc"][1] == 0 and rec["snr"].view(np.uint32)[0] == 0
    y = np.full((2, 16), -0.0, np.float32)
    y[1, 3] = 0.0
    rec = ref.records(ref.keys(y, 1, 1, 0.0, 1.0))
    assert rec["loc"][1] == 3 and rec["snr"].view(np.uint32)[1] == 0 and rec["snr"].view(np.uint32)[0] == 0x80000000
    y = np.full((2, 16), np.nan, np.float32)
    y[1, 7] = -np.inf
    rec = ref.records(ref.keys(y, 1, 1, 0.0, 1.0))
    assert rec["loc"][0] == 0xFFFFFFFF and rec["snr"][0] == -np.inf and rec["loc"][1] == 7 and rec["snr"][1] == -np.inf


def test_recorded_pulsar_is_found_by_the_yardstick():
    """L = 5, p = 36 .. 38, K = 4, mean 10, inv_sigma 0.5, Gaussian noise (10, 2) plus a 3.0-high, 4-sample pulse of period 37 + 11/31:
    the best record lies at (p, i) = (37, 11) with k = 2"""
    x = ref.pulsar(np.random.default_rng(7), 32 * 38, 37 + 11 / 31, 4, 3.0)
    peaks, _ = ref.search(x, 1, 36, 38, 5, 4, [10.0], [0.5])
    s, pi, i = ref.best(peaks)
    assert (s, 36 + pi, i) == (0, 37, 11) and peaks["loc"][s, pi, i] >> 24 == 2
    print("S/N", peaks["snr"][0, 1, 11], "p=36 max", peaks["snr"][0, 0].max(), "p=38 max", peaks["snr"][0, 2].max())
