"""CPU: clRationalResampler's bookkeeping (mi355_resampler_plan / _noutput_for need no device), its argument validation, and the
soundness of the yardstick itself (tests/resampler_ref.py): two independent restatements agree, and the tolerance the GPU tests
use holds with a factor two to spare for float32 sums in any order."""
import ctypes as C

import numpy as np
import pytest

import resampler_ref as ref

GRID = ref.grid()


def _plan(L_, L, M, K, c, n):
    nt, ph = C.c_int(-1), C.c_int(-1)
    used, need = C.c_longlong(-1), C.c_longlong(-1)
    rc = L_.mi355_resampler_plan(L, M, K, c, n, C.byref(nt), C.byref(used), C.byref(need), C.byref(ph))
    return rc, (nt.value, used.value, need.value, ph.value)


@pytest.mark.parametrize("case", GRID, ids=ref.case_id)
def test_the_two_restatements_agree(case):
    L, M, K = case
    h = ref.make_taps(K)
    for c in ref.phases(L):
        for n in (1, 65, 257):
            x = ref.make_input(L, M, K, c, n)
            y, used, c2 = ref.resample(h, L, M, x, n, c)
            z = ref.resample_by_stuffing(h, L, M, x, n, c)
            scale = max(float(np.abs(z).max()), 1e-300)
            assert float(np.abs(y - z).max()) <= 1e-12 * scale, (c, n)
            assert (used, c2) == ref.plan(L, M, K, c, n)[1::2]


def test_the_restatements_agree_for_complex_taps_and_the_rrc():
    for L, M in ref.COMPLEX_RATES:
        K = 4 * L + 3
        h = ref.make_taps(K, True)
        x = ref.make_input(L, M, K, L // 2, 257)
        y = ref.resample(h, L, M, x, 257, L // 2)[0]
        z = ref.resample_by_stuffing(h, L, M, x, 257, L // 2)
        assert float(np.abs(y - z).max()) <= 1e-12 * float(np.abs(z).max())
    h = ref.rrc(8.0, 8, 0.35, 89)
    assert abs(float(h.sum()) - 8.0) < 1e-5 and np.allclose(h, h[::-1]) and int(np.argmax(h)) == 44
    x = ref.make_input(8, 1, 89, 0, 257)
    y = ref.resample(h, 8, 1, x, 257, 0)[0]
    assert float(np.abs(y - ref.resample_by_stuffing(h, 8, 1, x, 257, 0)).max()) <= 1e-12 * float(np.abs(y).max())


@pytest.mark.parametrize("case", GRID, ids=ref.case_id)
def test_plan_and_noutput_for_equal_the_restatement(pkg, case):
    L_ = pkg.lib()
    L, M, K = case
    nt = ref.taps_per_arm(K, L)
    for c in ref.phases(L):
        for n in (0,) + ref.NOUT:
            rc, got = _plan(L_, L, M, K, c, n)
            assert rc == 0 and got == ref.plan(L, M, K, c, n), (c, n, got)
        for a in range(0, 3 * nt * L + 1):
            n = L_.mi355_resampler_noutput_for(L, M, K, c, a)
            assert n == ref.noutput_for(L, M, K, c, a), (c, a, n)
            # the largest n whose needed(n) fits: needed(n) <= a < needed(n + 1)
            assert ref.plan(L, M, K, c, n)[2] <= a < ref.plan(L, M, K, c, n + 1)[2], (c, a, n)


@pytest.mark.parametrize("L,M,K", [(160, 147, 3840), (1, 65536, 5)])
def test_positions_are_64_bit(pkg, L, M, K):
    L_ = pkg.lib()
    n = 1 << 40
    for c in ref.phases(L):
        rc, got = _plan(L_, L, M, K, c, n)
        assert rc == 0 and got == ref.plan(L, M, K, c, n)
        need = got[2]
        assert need > 1 << 39
        assert L_.mi355_resampler_noutput_for(L, M, K, c, need) == ref.noutput_for(L, M, K, c, need) >= n
        assert L_.mi355_resampler_noutput_for(L, M, K, c, need - 1) == ref.noutput_for(L, M, K, c, need - 1) < n


def test_validation(pkg):
    L_ = pkg.lib()
    INVALID, UNSUPPORTED = -1, -3
    for args in ((0, 1, 5, 0, 1), (1, 0, 5, 0, 1), (-2, 1, 5, 0, 1), (3, 2, 0, 0, 1), (3, 2, -1, 0, 1),  # L, M or K < 1
                 (3, 2, 5, 3, 1), (3, 2, 5, -1, 1), (1, 1, 5, 1, 1)):                                 # phase outside [0, L)
        assert _plan(L_, *args)[0] == INVALID, args
        assert L_.mi355_resampler_noutput_for(*args[:4], 100) == INVALID, args
    assert _plan(L_, 3, 2, 5, 0, -1)[0] == INVALID
    assert L_.mi355_resampler_noutput_for(3, 2, 5, 0, -1) == INVALID
    for args in ((65537, 1, 5, 0, 1), (1, 65537, 5, 0, 1)):
        assert _plan(L_, *args)[0] == UNSUPPORTED, args
    # the table: nt * L entries, 1048576 at the most
    assert _plan(L_, 1, 1, 1048576, 0, 1)[0] == 0
    assert _plan(L_, 1, 1, 1048577, 0, 1)[0] == UNSUPPORTED
    assert b"table entries" in L_.mi355_last_error()
    assert _plan(L_, 65536, 1, 16 * 65536, 0, 1)[0] == 0
    assert _plan(L_, 65536, 1, 16 * 65536 + 1, 0, 1)[0] == UNSUPPORTED     # nt = 17
    assert L_.mi355_resampler_noutput_for(65536, 1, 16 * 65536 + 1, 0, 100) == UNSUPPORTED
    assert _plan(L_, 65535, 1, 16 * 65535 + 1, 0, 1)[0] == UNSUPPORTED     # padding counts: 17 * 65535 > 1048576
    # NULL outputs are allowed; create refuses the same arguments before touching a device
    assert L_.mi355_resampler_plan(3, 2, 5, 0, 10, None, None, None, None) == 0
    h = C.c_void_p()
    taps = np.ones(5, np.float32)
    assert L_.mi355_resampler_create(None, 3, 2, taps.ctypes.data_as(C.c_void_p), 5, 0, C.byref(h)) == INVALID and not h.value
    assert L_.mi355_resampler_destroy(None) == 0
    assert L_.mi355_resampler_history(None) == INVALID and L_.mi355_resampler_ntaps(None) == INVALID
    assert L_.mi355_resampler_set_phase(None, 0) == INVALID


def test_python_classes_are_exported(pkg):
    assert issubclass(pkg.clInterpFIRFilter, pkg.clRationalResampler)
    assert pkg.clenabled.clRationalResampler is pkg.clRationalResampler


@pytest.mark.parametrize("case", GRID, ids=ref.case_id)
def test_the_tolerance_is_sound(case):
    """A float32 evaluation of the formula, summed forward, reversed and pairwise, stays below one half of bound()."""
    L, M, K = case
    n = 257
    for cplx in (False, True):
        if cplx and (L, M) not in ref.COMPLEX_RATES:
            continue
        h = ref.make_taps(K, cplx)
        for c in ref.phases(L):
            x = ref.make_input(L, M, K, c, n)
            want = ref.resample(h, L, M, x, n, c)[0]
            bnd = ref.bound(h, L, x, c, M, n)
            for name, y in ref.float32_orders(h, L, M, x, n, c).items():
                assert ref.worst(y, want, bnd) < 0.5, (name, cplx, c)
