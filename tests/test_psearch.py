"""clPulseSearch without a device: the yardstick tests/psearch_ref.py against hand-worked tiny cases (tie-break, +-0, NaN reach, a block of
nothing but NaN) and against the rule in words, the proof that a sequential sum is another function than the contract's tree, the sizes
of mi355_psearch_plan, every argument error of _plan / _create with a NULL context (which shows that the arguments are checked before
the context is touched), NULL handles, and the library's exports against the header.  The kernels are tested in
tests/test_psearch_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import psearch_ref as ref

NAMES = {"plan", "create", "destroy", "set_stats", "get_stats", "set_threshold", "history", "set_generic", "route", "work", "work_dev", "measure"}


def _plan(L, R, D, K, Tb, order):
    fi, hi, pb = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    rc = L.mi355_psearch_plan(R, D, K, Tb, order, C.byref(fi), C.byref(hi), C.byref(pb))
    return rc, (fi.value, hi.value, pb.value), L.mi355_last_error().decode()


def _create(L, R, D, K, Tb, order, ctx=None):
    h = C.c_void_p(1)
    rc = L.mi355_psearch_create(ctx, R, D, K, Tb, order, None, None, C.byref(h))
    assert rc != 0 and not h.value  # no handle comes back from a refused create
    return rc, L.mi355_last_error().decode()


def test_header_symbols_are_exported(pkg):
    """every mi355_psearch_* function the header declares is in the library, and they are the twelve of the contract"""
    with open(os.path.join(ROOT, "include", "mi355_clenabled.h")) as f:
        declared = set(re.findall(r"^[a-z][a-z ]*\*?\b(mi355_psearch_\w+)\(", f.read(), re.M))
    assert declared == {"mi355_psearch_" + n for n in NAMES}
    L = pkg.lib()
    for name in sorted(declared):
        assert getattr(L, name) is not None, name


def test_plan_sizes(pkg):
    L = pkg.lib()
    for R, D, K, Tb in ((64, 1024, 10, 1024), (1, 1, 1, 16), (3, 17, 13, 48), (4096, 4096, 13, (1 << 24) - 1)):
        for order in (ref.TRIAL_MAJOR, ref.TIME_MAJOR):
            assert _plan(L, R, D, K, Tb, order)[:2] == (0, ref.plan(R, D, K))
    assert _plan(L, 64, 1024, 10, 1024, 1)[1] == (65536, 511, 65536)
    assert L.mi355_psearch_plan(2, 8, 4, 16, 0, None, None, None) == 0  # any output pointer may be NULL


BAD = [
    # (R, D, K, Tb, order), message
    ((0, 8, 4, 16, 0), "num_rows must be 1 .. 4096"),
    ((4097, 8, 4, 16, 0), "num_rows must be 1 .. 4096"),
    ((2, 0, 4, 16, 0), "num_trials must be 1 .. 4096"),
    ((2, 4097, 4, 16, 0), "num_trials must be 1 .. 4096"),
    ((2, 8, 0, 16, 0), "num_widths must be 1 .. 13"),
    ((2, 8, 14, 16, 0), "num_widths must be 1 .. 13"),
    ((2, 8, 4, 15, 0), "block_len must be 16 .. 2^24 - 1"),
    ((2, 8, 4, 1 << 24, 0), "block_len must be 16 .. 2^24 - 1"),
    ((2, 8, 4, 16, 2), "order must be TRIAL_MAJOR (0) or TIME_MAJOR (1)"),
    ((2, 8, 4, 16, -1), "order must be TRIAL_MAJOR (0) or TIME_MAJOR (1)"),
]


@pytest.mark.parametrize("args,msg", BAD)
def test_argument_errors_come_before_the_context(pkg, args, msg):
    L = pkg.lib()
    rc, sizes, err = _plan(L, *args)
    assert (rc, sizes, err) == (-1, (0, 0, 0), "invalid argument: " + msg)
    assert _create(L, *args) == (-1, "invalid argument: " + msg)                              # NULL context
    assert _create(L, *args, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: " + msg)  # an invalid one is never touched


def test_create_checks_the_arguments_then_the_context(pkg):
    L = pkg.lib()
    assert _create(L, 2, 8, 4, 16, 1) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert _create(L, 4096, 4096, 13, (1 << 24) - 1, 0) == (-1, "invalid argument: NULL context")
    assert L.mi355_psearch_create(None, 2, 8, 4, 16, 1, None, None, None) == -1


def test_null_handles(pkg):
    L = pkg.lib()
    assert L.mi355_psearch_set_stats(None, None, None) == -1 and L.mi355_psearch_get_stats(None, None, None, 0) == -1
    assert L.mi355_psearch_set_generic(None, 1) == -1 and L.mi355_psearch_history(None) == -1
    assert L.mi355_psearch_set_threshold(None, 1.0) == -1
    assert L.mi355_psearch_work(None, 16, None, 0, None, None, 0, None) == -1
    assert L.mi355_psearch_work_dev(None, 16, None, 0, None, None, 0, None, None) == -1
    assert L.mi355_psearch_measure(None, 16, None, 0, 0, None, None) == -1
    assert L.mi355_psearch_route(None) == b"" and L.mi355_psearch_destroy(None) == 0


def test_python_class_refuses_before_a_context_exists(pkg):
    with pytest.raises(pkg.Mi355Error):
        pkg.clPulseSearch(1, 2, 0, 99, 2, 8, 14, 16)  # num_widths; device 99 is never looked for
    with pytest.raises(ValueError):
        pkg.clPulseSearch(1, 2, 0, 99, 2, 8, 4, 16, 1, np.zeros(5, np.float32))
    with pytest.raises(TypeError):
        pkg.clPulseSearch(1, 2, 0, 99, 2, 8, 4, 16, 1, None, np.zeros(16, np.float64))
    with pytest.raises(ValueError):
        pkg.clPulseSearch(1, 2, 0, 99, 2, 8, 4, 16, max_cands=-1)


def test_gains_are_the_nearest_float32():
    for k in range(13):
        assert ref.c(k) == np.float32(2.0 ** (-k / 2)), k
    assert ref.c(1).view(np.uint32) == 0x3F3504F3 and ref.c(2) == np.float32(0.5) and ref.c(3).view(np.uint32) == 0x3F3504F3 - (1 << 23)


def _rec(snr, k, t):
    return np.array((snr, (k << 24) | t), ref.PEAK)


def test_ref_hand_worked_peaks():
    one = np.float32(1.0)
    r2 = ref.c(1)
    # ones: snr_0 = 1 everywhere, snr_1 = 2 c_1 = 1.414 everywhere: the wider boxcar wins, at the first sample
    pk = ref.peaks(np.ones((1, 17), np.float32), 2, 16, 16)
    assert pk.shape == (1, 1) and pk[0, 0] == _rec(np.float32(2.0) * r2, 1, 0)
    # an impulse: the narrowest boxcar wins, where the impulse is
    x = np.zeros((1, 19), np.float32)
    x[0, 5] = 4.0
    assert ref.peaks(x, 3, 16, 16)[0, 0] == _rec(4.0, 0, 5)
    # an exact tie between widths: {1, 1} gives snr_0 = 1 twice and snr_2 over {1, 1, 1, 1} = 4 / 2 = 2 = snr_0 of a lone 2 elsewhere
    x = np.zeros((1, 19), np.float32)
    x[0, 2:6] = 1.0
    x[0, 12] = 2.0
    assert ref.peaks(x, 3, 16, 16)[0, 0] == _rec(2.0, 0, 12)  # the smallest k of the equals, although t = 2 comes first
    x[0, 12] = 0.0
    x[0, 1] = 0.0
    assert ref.peaks(x, 3, 16, 16)[0, 0] == _rec(2.0, 2, 2)
    # all zero: every snr is +0, the smallest k and t
    assert ref.peaks(np.zeros((1, 19), np.float32), 3, 16, 16)[0, 0] == _rec(0.0, 0, 0)
    # mean and inv_sigma: (x - m 2^k) g c_k
    pk = ref.peaks(np.full((1, 17), 3.0, np.float32), 2, 16, 16, [one], [np.float32(0.5)])
    assert pk[0, 0] == _rec(np.float32(4.0) * (np.float32(0.5) * r2), 1, 0)


def test_ref_plus_zero_is_above_minus_zero():
    x = np.full((1, 17), -0.0, np.float32)
    pk = ref.peaks(x, 2, 16, 16)
    assert np.signbit(pk["snr"][0, 0]) and pk["snr"][0, 0] == 0 and pk["loc"][0, 0] == 0  # every snr is -0
    x[0, 6] = 0.0
    pk = ref.peaks(x, 2, 16, 16)  # snr_0[6] = +0 and snr_1[5] = snr_1[6] = +0: +0 wins, then the smallest k
    assert not np.signbit(pk["snr"][0, 0]) and pk["loc"][0, 0] == 6
    assert np.array_equal(pk, ref.peaks_lexicographic(x, 2, 16, 16))


def test_ref_nan_reach_and_empty_block():
    rng = np.random.default_rng(3)
    K, n, t0 = 4, 32, 10
    x = rng.standard_normal((1, n + ref.history(K))).astype(np.float32)
    x[0, t0] = np.nan
    s = ref.snr(x, K, n)
    for k in range(K):
        t = np.arange(n)
        assert np.array_equal(np.isnan(s[k, 0]), (t > t0 - (1 << k)) & (t <= t0)), k  # exactly t0 - 2^k < t <= t0
    # a NaN run over a whole block and its look-ahead: {-Inf, 0xFFFFFFFF}; the next block is untouched beyond the reach
    x = rng.standard_normal((2, 33)).astype(np.float32)
    x[1, :17] = np.nan
    pk = ref.peaks(x, 2, 16, 32)
    assert pk[0, 1] == np.array((-np.inf, 0xFFFFFFFF), ref.PEAK) and np.isfinite(pk["snr"][0, 0]) and np.isfinite(pk["snr"][1]).all()
    assert (pk["loc"][1, 1] & 0xFFFFFF) != 0  # t = 16 of the call is the one sample of block 1 that the run reaches
    assert np.array_equal(pk, ref.peaks_lexicographic(x, 2, 16, 32))
    # +Inf lands where the formula puts it
    x = rng.standard_normal((1, 19)).astype(np.float32)
    x[0, 7] = np.inf
    assert ref.peaks(x, 3, 16, 16)[0, 0] == _rec(np.inf, 0, 7)


@pytest.mark.parametrize("kind", ["gaussian", "integers"])
def test_ref_key_order_is_the_rule_in_words(kind):
    rng = np.random.default_rng(11)
    K, Tb, n, S = 5, 16, 48, 3
    T = n + ref.history(K)
    x = rng.standard_normal((S, T)).astype(np.float32) if kind == "gaussian" else rng.integers(0, 4, (S, T)).astype(np.float32)
    mean = np.full(S, 1.5 if kind == "integers" else 0.25, np.float32)
    isg = np.array([1.0, 0.5, 2.0], np.float32)
    pk = ref.peaks(x, K, Tb, n, mean, isg)
    assert np.array_equal(pk, ref.peaks_lexicographic(x, K, Tb, n, mean, isg))
    if kind == "integers":  # the fixture is one with exact ties, or it would not exercise the tie-break
        s = ref.snr(x, K, n, mean, isg).reshape(K, S, n // Tb, Tb)
        assert ((s == pk["snr"].T[None, :, :, None]).sum(axis=(0, 3)) > 1).any()


def test_a_sequential_sum_is_not_the_tree():
    """the contract is the balanced tree: on Gaussian data a left-to-right sum of the same samples has other bits"""
    rng = np.random.default_rng(1)
    K, n = 10, 4096
    x = (rng.standard_normal(n + ref.history(K)) * 3 + 10).astype(np.float32)
    lv = ref.tree(x, K)
    assert np.array_equal(lv[1][:n], ref.sequential(x, 1)[:n])  # two terms: one addition either way
    for k, least in ((2, 0.05), (5, 0.5), (9, 0.8)):
        assert np.mean(lv[k][:n] != ref.sequential(x, k)[:n]) > least, k
    cs = np.cumsum(x, dtype=np.float32)
    w = 1 << 9
    diff = cs[w - 1:w - 1 + n] - np.concatenate([[np.float32(0)], cs[:n - 1]]).astype(np.float32)
    assert np.mean(lv[9][:n] != diff) > 0.9


def test_ref_candidates_and_orders():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 40)).astype(np.float32)
    pk = ref.peaks(x, 4, 16, 32)
    thr = np.sort(pk["snr"].reshape(-1))[-4]
    cand = ref.candidates(pk, thr)
    assert cand.shape == (4, 4) and (cand[:, 0].view(np.float32) >= thr).all()
    for snr_bits, loc, s, b in cand:
        assert pk["loc"][b, s] == loc and pk["snr"][b, s].view(np.uint32) == snr_bits
    assert ref.candidates(pk, np.inf).shape == (0, 4) and ref.candidates(pk, -np.inf).shape == (12, 4)
    tm = ref.to_order(x, ref.TIME_MAJOR)
    assert tm.shape == (240,) and tm[6 * 3 + 2] == x[2, 3]
    tr = ref.to_order(x, ref.TRIAL_MAJOR, 45)
    assert tr.shape == (5 * 45 + 40,) and tr[2 * 45 + 3] == x[2, 3] and np.isnan(tr[40:45]).all()
    m, g = ref.measure(np.array([[1.0, 3.0, 1.0, 3.0], [2.0, 2.0, 2.0, 2.0]], np.float32), 4)
    assert np.array_equal(m, [2.0, 2.0]) and np.array_equal(g, [1.0, 0.0])


def test_ref_pulse_scene_peaks_where_the_pulse_is():
    """the end-to-end fixture of tests/test_psearch_gpu.py, on the CPU: the two references chained put the global maximum on the
    injected (row, trial, width 8, time)"""
    import dedisp_ref
    sc = ref.pulse_scene()
    y = dedisp_ref.dedisperse(sc["x"], sc["tab"], sc["n_dd"], dedisp_ref.TRIAL_MAJOR)  # [r][d][t]
    pk = ref.peaks(y.reshape(sc["R"] * sc["D"], sc["n_dd"]), sc["K"], sc["Tb"], sc["n"], None, sc["inv_sigma"])
    b, s = np.unravel_index(np.argmax(pk["snr"]), pk.shape)
    assert (s, b) == (sc["r0"] * sc["D"] + sc["d0"], sc["t0"] // sc["Tb"])
    assert pk["loc"][b, s] == (3 << 24) | (sc["t0"] % sc["Tb"]) and 40 < pk["snr"][b, s] < 50
    assert np.sort(pk["snr"].reshape(-1))[-2] < pk["snr"][b, s] - 3  # by a margin: no other record comes near
