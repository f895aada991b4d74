"""CPU: clFreqXlatingFIRFilter's bookkeeping that needs no device -- mi355_xlate_plan against the formula, the two forms of the
yardstick (tests/xlate_ref.py) against each other, the 64-bit phase arithmetic in Python integers, and the argument errors that are
reported before a context is touched."""
import ctypes as C

import numpy as np
import pytest

import xlate_ref as ref


def _plan(L, D, K, n):
    nin, hist = C.c_longlong(-1), C.c_int(-1)
    rc = L.mi355_xlate_plan(D, K, n, C.byref(nin), C.byref(hist))
    return rc, nin.value, hist.value


def test_plan_against_the_formula(pkg):
    L = pkg.lib()
    for D, K, n in [(1, 1, 1), (2, 7, 5), (16, 65, 257), (64, 512, 1 << 20), (25, 131, 0), (3, 3000, 12345),
                    (16, 65, 1 << 40), (7, 9, (1 << 62) // 7), (1, 2000000000, (1 << 62))]:
        assert _plan(L, D, K, n) == (0, ref.plan(D, K, n), K), (D, K, n)
    assert _plan(L, 16, 65, 1 << 40)[1] == (1 << 44) + 64  # needs 64 bits
    assert L.mi355_xlate_plan(8, 33, 10, None, None) == 0  # either pointer may be NULL
    for D, K, n in [(0, 5, 1), (-1, 5, 1), (4, 0, 1), (4, 5, -1)]:
        rc, nin, hist = _plan(L, D, K, n)
        assert (rc, nin, hist) == (-1, 0, 0), (D, K, n)
        assert b"invalid argument" in L.mi355_last_error()
    assert _plan(L, 2, 5, (1 << 61) + 1)[0] == -3 and _plan(L, 7, 9, (1 << 62) // 7 + 1)[0] == -3


@pytest.mark.parametrize("D,K,f,cplx", [(1, 1, 0.0, False), (2, 7, 12500.0, False), (5, 33, -250000.0, True), (16, 65, 123456.789, False),
                                        (3, 8, 500000.0, True), (8, 9, -500000.0, False), (25, 131, 999999.0 / np.pi, True)])
def test_bandpass_decimate_rotate_is_mix_filter_decimate(D, K, f, cplx):
    """form 1 with unrounded band-pass taps and the integer phase against form 2 with the exact f / fs: pins every sign"""
    fs = 1.0e6
    n = 300
    h = ref.make_taps(K, cplx, seed=K)
    x = ref.make_input(ref.plan(D, K, n), seed=D)
    y1, _ = ref.xlate(ref.bandpass64(h, f, fs), x, D, n, 0, ref.inc_of(f, D, fs))
    y2 = ref.xlate_mix(h, f, fs, x, D, n)
    assert np.abs(y1 - y2).max() <= 1e-9 * np.abs(y2).max()


def test_a_tone_at_the_centre_frequency_lands_at_dc():
    fs, f, D, K = 48000.0, -7000.0, 4, 16
    n = 64
    t = np.arange(ref.plan(D, K, n)) - (K - 1)
    x = np.exp(2j * np.pi * f / fs * t)
    h = np.full(K, 1.0 / K, np.float32)
    y, _ = ref.xlate(ref.bandpass64(h, f, fs), x, D, n, 0, ref.inc_of(f, D, fs))
    assert np.abs(y - 1.0).max() <= 1e-6  # (the input is rounded to float32)


def test_phase_bookkeeping_in_integers():
    fs, D = 1.0e6, 16
    for f in (0.0, 1.0, -1.0, 250000.0, -500000.0, 500000.0, 123456.789, 1e-3, -1e-3, 1e6 / 3):
        inc = ref.inc_of(f, D, fs)
        assert 0 <= inc < ref.TWO64 and ref.check_inc(inc, f, D, fs)
        assert (inc + ref.inc_of(-f, D, fs)) % ref.TWO64 == 0  # negative frequencies wrap
    assert ref.inc_of(0.0, D, fs) == 0 and ref.inc_of(fs / D, D, fs) == 0 and ref.inc_of(fs / (2 * D), D, fs) == 1 << 63
    assert ref.inc_of(-1e-3, D, fs) > (1 << 63)  # a small negative frequency is a large unsigned increment
    inc = ref.inc_of(123456.789, D, fs)
    whole = ref.phasor(0, inc, 200)
    # a call boundary: the carried phase continues the sequence bit for bit
    for cut in (1, 63, 64, 65, 199):
        carried = (inc * cut) % ref.TWO64
        assert np.array_equal(whole[cut:], ref.phasor(carried, inc, 200 - cut))
    # skip: 2^40 outputs later, exact in integers
    far = (inc * (1 << 40)) % ref.TWO64
    p = ref.phasor(far, inc, 3)
    want = [np.exp(-2j * np.pi * (((inc * ((1 << 40) + m)) % ref.TWO64) / 2.0 ** 64)) for m in range(3)]
    assert np.abs(p - np.array(want)).max() <= 1e-15
    # wrap-around: the accumulator passes 2^64 and the phasor does not jump
    near = ref.TWO64 - 3
    q = ref.phasor(near, 2, 4)  # phases -3, -1, +1, +3 units of 2^-64 turns
    assert np.abs(q - 1.0).max() <= 1e-15 and q[0].imag > 0 > q[3].imag
    # a retune keeps the phase: the first output after it continues from the accumulated value with the new increment
    inc2 = ref.inc_of(-200000.0, D, fs)
    n1 = 77
    P1 = (inc * n1) % ref.TWO64
    assert ref.phasor(P1, inc2, 1)[0] == ref.phasor(0, inc, n1 + 1)[n1]
    assert ref.phasor(P1, inc2, 2)[1] == ref.phasor((P1 + inc2) % ref.TWO64, 0, 1)[0]


def test_argument_errors_need_no_device(pkg):
    L = pkg.lib()
    h = C.c_void_p()
    taps = np.ones(5, np.float32)
    tp = C.c_void_p(taps.ctypes.data)

    def create(D, t, K, fs, freqs, ctx=None):
        f = np.asarray(freqs, np.float64)
        fp = f.ctypes.data_as(C.POINTER(C.c_double)) if freqs is not None else None
        rc = L.mi355_xlate_create(ctx, D, t, K, 0, fs, fp, 0 if freqs is None else f.size, 0, C.byref(h))
        assert not h.value
        return rc, L.mi355_last_error().decode()

    assert create(0, tp, 5, 1e6, [0.0]) == (-1, "invalid argument: decimation must be >= 1")
    assert create(4, tp, 0, 1e6, [0.0]) == (-1, "invalid argument: at least one tap")
    assert create(4, None, 5, 1e6, [0.0]) == (-1, "invalid argument: taps is NULL")
    assert create(4, tp, 5, 1e6, [])[1] == "invalid argument: at least one centre frequency"
    assert create(4, tp, 5, 1e6, None)[0] == -1
    for fs in (0.0, -1.0, float("inf"), float("nan")):
        assert create(4, tp, 5, fs, [0.0]) == (-1, "invalid argument: the sample rate must be finite and > 0")
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert create(4, tp, 5, 1e6, [0.0, bad]) == (-1, "invalid argument: a centre frequency is not finite")
    assert create(4, tp, 5, 1e6, [0.0] * 4097)[0] == -3
    assert create(4, tp, 5, 1e6, [0.0]) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert L.mi355_xlate_create(None, 4, tp, 5, 0, 1e6, None, 1, 0, None) == -1
    # NULL handles
    assert L.mi355_xlate_set_center_freq(None, 0, 1.0) == -1 and L.mi355_xlate_skip(None, 1) == -1
    assert L.mi355_xlate_set_generic(None, 1) == -1 and L.mi355_xlate_set_phase(None, 0, 1) == -1
    assert L.mi355_xlate_get_state(None, 0, None, None) == -1 and L.mi355_xlate_work_dev(None, 1, None, None, None) == -1
    assert L.mi355_xlate_ntaps(None) == -1 and L.mi355_xlate_num_channels(None) == -1 and L.mi355_xlate_decimation(None) == -1
    assert L.mi355_xlate_route(None) == b"" and L.mi355_xlate_destroy(None) == 0
