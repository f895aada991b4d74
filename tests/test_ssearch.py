"""clSpectralSearch without a device: the index r(k, j, h) of the yardstick tests/ssearch_ref.py against a literal evaluation with
Python integers, the proof that descending j and level-first sums are other functions than the contract's order, the recorded pulse
train below clPeriodSearch's 16-sample floor, the spectrum bound against planted faults of the half-length algorithm (a float32 numpy
restatement, on the inputs tests/test_ssearch_gpu.py uses), the library's exports against the header, mi355_ssearch_plan / _freq and
every create-time refusal through the C ABI with a NULL context (which shows that the arguments are checked before the context is
touched).  The kernels are tested in tests/test_ssearch_gpu.py."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import psearch_ref
import ssearch_ref as ref

NAMES = {"plan", "create", "destroy", "set_stats", "get_stats", "set_threshold", "set_generic", "route", "fft_route", "work", "work_dev", "freq"}
INVALID, UNSUPPORTED = -1, -3


@pytest.mark.parametrize("Nb", [128, 1024])
def test_index_against_python_integers(Nb):
    """integer-valued spectra, where every order of summation is exact: s_h[k] = sum over j <= 2^h of w[round-half-up(k j / 2^h)],
    evaluated literally; r <= k, k = 0 and k = Nb - 1 included"""
    rng = np.random.default_rng(Nb)
    w = rng.integers(0, 64, Nb).astype(np.float32)
    lv = ref.levels(w, ref.MAX_H)
    wi = [int(v) for v in w]
    for h in range(ref.MAX_H + 1):
        for k in sorted({0, 1, 2, 3, 5, Nb // 3, Nb // 2, Nb - 2, Nb - 1} | set(int(v) for v in rng.integers(0, Nb, 24))):
            idx = [(k * j * 2 + (1 << h)) // (2 << h) for j in range(1, (1 << h) + 1)]  # floor(k j / 2^h + 1/2) in integers
            assert all(0 <= i <= k for i in idx) and idx[-1] == k
            assert int(lv[h][k]) == sum(wi[i] for i in idx), (h, k)
            for j in range(1, 1 << h, 2):
                assert ref.r(k, j, h) == (k * j * 2 + (1 << h)) // (2 << h) <= k
    assert all(int(lv[h][0]) == (1 << h) * wi[0] for h in range(ref.MAX_H + 1))


def test_other_orders_are_other_functions():
    """the contract's figures on the CPU: about two thirds of the 2048 bins of a noise spectrum change at H = 5"""
    w = np.random.default_rng(1).exponential(1.0, 2048).astype(np.float32)
    a = ref.levels(w, 5)[5]
    d, l = ref.levels_descending(w, 5)[5], ref.levels_level_first(w, 5)[5]
    nd, nl = int((a.view(np.uint32) != d.view(np.uint32)).sum()), int((a.view(np.uint32) != l.view(np.uint32)).sum())
    print("descending j changes %d bins of 2048, level-first %d" % (nd, nl))
    assert nd > 1000 and nl > 1000
    assert np.allclose(a, d, rtol=1e-5) and np.allclose(a, l, rtol=1e-5)


def test_recorded_pulse_train_is_found_by_the_yardstick():
    """N = 4096, one-sample pulses 4 sigma high every 12.8 samples (below the FFA's 16-sample floor) in unit Gaussian noise: the
    fundamental lies on bin 320, harmonics 2 .. 6 on 640 .. 1920, so level 2 at k = 1280 holds four of them and is the best record of
    all.  Recorded margin: S/N 324.5 at (h, k) = (2, 1280) against 241.3 for the best of level 1 (k = 640), 228.9 for level 3 and 189.9
    for level 0 -- the winner leads by a third."""
    x = ref.pulse_train(np.random.default_rng(12), 4096, 12.8, 4.0)[None]
    g = psearch_ref.measure(x, 4096)[1].astype(np.float32)
    w = ref.spectrum64(x, g, 1).astype(np.float32)
    pk = ref.peaks(w, 5, 16)
    assert ref.best(pk, 16) == (0, 2, 1280)
    s = ref.snr(w, 5)[:, 0]
    top = [float(s[h].max()) for h in range(6)]
    print("S/N per level", top)
    assert top[2] == pk["snr"].max() and top[2] > 1.3 * max(top[:2] + top[3:])
    assert 0.9 < w[0, 1:].mean() < 1.1 + 6 * 16.0 * 16.0 / 2048  # white noise gives a mean of 1; the six harmonics add their share


@pytest.mark.parametrize("N", [256, 4096])
def test_bound_separates_the_algorithm_from_planted_faults(N):
    """the float32 restatement of the half-length algorithm uses a small part of the bound; each planted fault exceeds it on every
    series that is not zero"""
    for name, (x, g) in ref.series_cases(N).items():
        used = ref.spectrum_used(ref.spectrum32(x, g, 3), x, g, 3)
        print(N, name, "used", used)
        assert used <= 1.0
        for s in range(x.shape[0]):
            for fault in ("twiddle_sign", "unconjugated", "off_by_one"):
                u = ref.spectrum_used(ref.spectrum32(x[s:s + 1], g[s:s + 1], 3, fault), x[s:s + 1], g[s:s + 1], 3)
                assert (u > 1.0) if x[s].any() else (u == 0.0), (name, s, fault, u)
    x, g = ref.series_cases(N)["tones"]
    w = ref.spectrum32(x, g, 3)
    assert (w[:, :3].view(np.uint32) == 0).all() and 0.9 < w[0].mean() < 1.1


def test_key_order_of_the_yardstick():
    """a constant spectrum: every level's snr is (2^h c - 2^h) c_h, so with c = 1 all are 0 and every tie goes to h = 0 and the smallest
    k; +0 above -0; NaN never takes part"""
    pk = ref.peaks(np.ones((2, 128), np.float32), 5, 16)
    assert (pk["loc"] == 0).all() and (pk["snr"].view(np.uint32) == 0).all()
    w = np.full((1, 128), np.nan, np.float32)
    pk = ref.peaks(w, 5, 16)
    assert (pk["loc"] == 0xFFFFFFFF).all() and np.isneginf(pk["snr"]).all()
    w = np.ones((1, 128), np.float32)
    w[0, 0] = np.nan  # k = 0 at every level, and r(k, j, h) = 0 for the k near 0 only
    pk = ref.peaks(w, 5, 128)
    assert pk["loc"][0, 0] == 1 and pk["snr"][0, 0] == 0  # (h, k) = (0, 1): the smallest k whose sum does not read bin 0


def test_header_symbols_are_exported(pkg):
    with open(os.path.join(ROOT, "include", "mi355_clenabled.h")) as f:
        declared = set(re.findall(r"^[a-z][a-z ]*\*?\b(mi355_ssearch_\w+)\(", f.read(), re.M))
    assert declared == {"mi355_ssearch_" + n for n in NAMES}
    L = pkg.lib()
    for name in sorted(declared):
        assert getattr(L, name) is not None, name
    assert callable(pkg.ssearch_freq) and pkg.SSEARCH_SERIES == 0 and pkg.SSEARCH_SPECTRUM == 1


def test_freq_through_the_c_abi(pkg):
    L = pkg.lib()
    for N, ts, h, k in [(4096, 1e-3, 2, 1280), (256, 1.0, 0, 127), (1 << 22, 64e-6, 5, (1 << 21) - 1), (1 << 20, 1e-3, 3, 0), (4096, 0.5, 5, 1)]:
        want = Fraction(k) / (Fraction(1 << h) * N * Fraction(ts))
        got = L.mi355_ssearch_freq(N, ts, h, k)
        assert abs(Fraction(got) - want) <= want * Fraction(3, 1 << 53), (N, ts, h, k)
        assert pkg.ssearch_freq(N, ts, h, k) == got
    assert 1.0 / pkg.ssearch_freq(4096, 1e-3, 2, 1280) == pytest.approx(12.8e-3, rel=1e-15)
    for bad in [(255, 1.0, 0, 0), (128, 1.0, 0, 0), (1 << 23, 1.0, 0, 0), (4096, 1.0, -1, 0), (4096, 1.0, 6, 0), (4096, 1.0, 0, -1),
                (4096, 1.0, 0, 2048), (4096, 0.0, 0, 1), (4096, -1.0, 0, 1), (4096, float("nan"), 0, 1), (4096, float("inf"), 0, 1)]:
        assert np.isnan(L.mi355_ssearch_freq(*bad)), bad
        with pytest.raises(ValueError):
            pkg.ssearch_freq(*bad)


def _plan(L, *shape):
    out = [C.c_longlong(-1) for _ in range(3)]
    rc = L.mi355_ssearch_plan(*shape, *[C.byref(o) for o in out])
    return rc, tuple(o.value for o in out), L.mi355_last_error().decode()


def test_plan_sizes(pkg):
    L = pkg.lib()
    rc, (nb, rec, scratch), _ = _plan(L, 1024, 1 << 20, 5, 1024, 8, ref.SERIES)
    assert rc == 0 and nb == 1 << 19 and rec == 512
    assert 6 << 20 <= scratch <= 512 << 20  # at least one series' Z and w, bounded however many series there are
    rc, (nb, rec, scratch), _ = _plan(L, 3, 256, 0, 16, 1, ref.SERIES)
    assert rc == 0 and (nb, rec) == (128, 8) and scratch >= 3 * 6 * 256
    rc, (nb, rec, scratch), _ = _plan(L, 2, 16384, 5, 8192, 8191, ref.SPECTRUM)
    assert rc == 0 and (nb, rec, scratch) == (8192, 1, 0)
    assert L.mi355_ssearch_plan(1, 256, 0, 16, 1, 0, None, None, None) == 0
    assert pkg.clSpectralSearch.plan(3, 4096, 5, 16)[:2] == (2048, 128)


REFUSED = [
    ((0, 4096, 5, 16, 1, 0), INVALID, "num_series"),
    (((1 << 20) + 1, 4096, 5, 16, 1, 0), INVALID, "num_series"),
    ((1, 128, 5, 16, 1, 0), INVALID, "power of two"),
    ((1, 4095, 5, 16, 1, 0), INVALID, "power of two"),
    ((1, 1 << 23, 5, 16, 1, 0), INVALID, "power of two"),
    ((1, 4096, -1, 16, 1, 0), INVALID, "num_folds"),
    ((1, 4096, 6, 16, 1, 0), INVALID, "num_folds"),
    ((1, 4096, 5, 8, 1, 0), INVALID, "block_bins"),
    ((1, 4096, 5, 48, 1, 0), INVALID, "block_bins"),
    ((1, 4096, 5, 4096, 1, 0), INVALID, "block_bins"),
    ((1, 4096, 5, 16, 0, 0), INVALID, "k_lo"),
    ((1, 4096, 5, 16, 2048, 0), INVALID, "k_lo"),
    ((1, 4096, 5, 16, 1, 2), INVALID, "input_kind"),
    ((1, 4096, 5, 16, 1, -1), INVALID, "input_kind"),
    ((1 << 20, 1 << 22, 5, 16, 1, 0), UNSUPPORTED, "2^40"),   # 2^44 bytes of input
    ((1 << 20, 1 << 20, 5, 16, 1, 1), UNSUPPORTED, "2^40"),   # 2^41 bytes of spectra
]


@pytest.mark.parametrize("shape,code,word", REFUSED)
def test_refusals_without_a_device(pkg, shape, code, word):
    L = pkg.lib()
    rc, sizes, msg = _plan(L, *shape)
    assert rc == code and sizes == (0, 0, 0) and word in msg, msg
    h = C.c_void_p(1)
    rc = L.mi355_ssearch_create(None, *shape, None, C.byref(h))  # a NULL context: refused for the shape, not for the context
    assert rc == code and not h.value and word in L.mi355_last_error().decode()
    with pytest.raises(pkg.Mi355Error):
        pkg.clSpectralSearch(0, 0, 0, 0, *shape)


def test_limits_are_accepted_and_null_handles_refused(pkg):
    L = pkg.lib()
    assert _plan(L, 1, 1 << 22, 5, 1 << 21, (1 << 21) - 1, 0)[0] == 0 and _plan(L, 1 << 20, 256, 0, 16, 1, 0)[0] == 0
    assert _plan(L, 1 << 20, 1 << 18, 5, 16, 1, 0)[0] == 0 and _plan(L, 1 << 20, 1 << 19, 5, 16, 1, 1)[0] == 0  # 2^40 bytes exactly
    h = C.c_void_p(1)
    assert L.mi355_ssearch_create(None, 1, 256, 0, 16, 1, 0, None, C.byref(h)) == INVALID and not h.value  # now it is the context
    assert "context" in L.mi355_last_error().decode()
    assert L.mi355_ssearch_create(None, 1, 256, 0, 16, 1, 0, None, None) == INVALID
    assert L.mi355_ssearch_destroy(None) == 0 and L.mi355_ssearch_route(None) == b"" and L.mi355_ssearch_fft_route(None) == b""
    assert L.mi355_ssearch_set_generic(None, 1) == INVALID and L.mi355_ssearch_set_stats(None, None) == INVALID
    assert L.mi355_ssearch_set_threshold(None, 1.0) == INVALID and L.mi355_ssearch_get_stats(None, None, 0) == INVALID
    assert L.mi355_ssearch_work(None, None, 0, None, None, None, 0, None) == INVALID
    assert L.mi355_ssearch_work_dev(None, None, 0, None, None, None, 0, None, None) == INVALID
    with pytest.raises(ValueError):
        pkg.clSpectralSearch(0, 0, 0, 0, 1, 4096, 5, 16, max_cands=-1)
