"""CPU: the per-frame, per-lag error bounds of clxcorrelate_fft_vcf (tests/fft_ref.py: xcorr_bound_check against xcorr_frames64) are fixed
here, on float32 evaluations that run on the CPU, and never on a GPU result.

The rule is that of tests/test_fft_ref.py: every CPU float32 evaluation stays at or under HALF of each bound; (a, b) = XCORR_MULT[kind] are
the smallest integers at or above twice the largest figure measured here.  The evaluation is a complex64 correlator -- forward transforms
(time series), a complex64 product X0 conj(Xs), the unscaled inverse transform, sqrt(re re + im im) in float, the half swap -- over
  the radix-2 complex64 FFT of tests/test_fft_ref.py (_fft2_c64, one table W_N^k rounded to float),
  scipy's complex64 pocketfft,
  and, for the composed route, the emulations of clFFT's other structures (_mr_c64, _mr_tile_c64, _chirpz_c64) at the lengths the GPU
  cases use (tests/test_xcorr_bounds_gpu.py); their inverse is conj(forward(conj(.))), which rounds as a conjugated table does.
Inputs: every ordered pair of the four kinds of fft_inputs (a seed per operand; the impulse and tone sets do not depend on it, so impulses
meet impulses at lag 0 and a tone meets the same tone), the autocorrelation of every kind, a delayed copy under mixed per-frame scales;
spectra and time series.  Not in the grid, and outside the form: time-series tones whose bins differ -- their product cancels, and a
float32 transform of a tone may leave its whole error in ONE other bin, which then meets the other tone's peak ('Tolerances').

Then the planted errors, each of which conftest.relerr <= 1e-5 (one scale per call) lets through and the bounds must not: the twiddle table
rounded to 16 significand bits, one table entry off by 3e-6, and, in a `mixed` call, the quietest live frame of one signal zeroed, left
unswapped, or computed as X0 Xs without the conjugate.  Every test prints its figures (pytest -s)."""
import numpy as np
import pytest

from conftest import relerr
from fft_ref import MR_PLANS, MR_TILE_PLANS, XCORR_MULT, fft_inputs, xcorr_bound_check, xcorr_frames64
from test_fft_ref import _c64, _chirpz_c64, _fft2_c64, _mr_c64, _mr_tile_c64, _table

KINDS = ["mixed", "impulses", "tones", "tone_noise"]
ITYPES = [1, 2]
TOL_OLD = 1e-5


def _frames(n):
    return n + 1 if n <= 64 else 24  # short lengths: the identity / one tone per bin and one more; the rest: edges and seeded positions


def _swap(r):
    n = r.shape[1]
    return np.concatenate([r[:, n // 2:], r[:, :n // 2]], axis=1)


def _xcorr_c64(itype, x0, xs, fwd, inv, conj=True, swap=True):
    """the correlator in complex64 over the transforms fwd / inv (rows of a (frames, n) array; inv unscaled)"""
    X0, Xs = (_c64(x0), _c64(xs)) if itype == 1 else (_c64(fwd(x0)), _c64(fwd(xs)))
    r = _c64(inv(_c64(X0 * (np.conj(Xs) if conj else Xs))))
    re, im = r.real.astype(np.float32), r.imag.astype(np.float32)
    mag = np.sqrt(re * re + im * im)
    assert mag.dtype == np.float32
    return _swap(mag) if swap else mag


def _radix2(n, **table):
    tab = _table(n, **table)
    return (lambda x: _fft2_c64(x, tab)), (lambda p: _fft2_c64(p, tab, inverse=True))


def _pocketfft():
    sfft = pytest.importorskip("scipy.fft")
    return (lambda x: sfft.fft(_c64(x), axis=1)), (lambda p: sfft.ifft(_c64(p), axis=1, norm="forward"))


def _via_forward(f):
    return f, (lambda p: np.conj(f(np.conj(_c64(p)))))


def _pairs(n, frames):
    """(label, reference operand, signal operand) of every ordered pair, the autocorrelations and the delayed copy"""
    ref = {k: fft_inputs(k, n, frames, 100 * n + i) for i, k in enumerate(KINDS)}
    sig = {k: fft_inputs(k, n, frames, 100 * n + 10 + i) for i, k in enumerate(KINDS)}
    out = [("%s x %s" % (k0, k1), ref[k0], sig[k1]) for k0 in KINDS for k1 in KINDS]
    out += [("auto %s" % k, ref[k], ref[k].copy()) for k in KINDS]
    d = max(1, n // 3)
    out.append(("mixed delayed by %d" % d, ref["mixed"], np.roll(ref["mixed"], d, axis=1)))
    return out


def _measure(name, n, frames, fwd, inv, kind, itypes=ITYPES, only=None):
    """the largest used fractions over the input grid (only: the pairs of that list), printed in units (the fraction times the multiple)"""
    a, b = XCORR_MULT[kind]
    worst = [0.0, 0.0]
    for itype in itypes:
        top = [0.0, "", 0.0, ""]
        for label, x0, xs in _pairs(n, frames):
            if only and label not in only:
                continue
            got = _xcorr_c64(itype, x0, xs, fwd, inv)
            (mag, sc), = xcorr_frames64(n, itype, [x0, xs])
            fl, fr = xcorr_bound_check(got, mag, sc, n, itype, kind, check=False)
            assert np.isfinite(fl) and np.isfinite(fr), (name, n, itype, label)  # (inf: a zero frame that did not come out as zeros)
            if fl > top[0]:
                top[:2] = [fl, label]
            if fr > top[2]:
                top[2:] = [fr, label]
        print("%s n %d %s: %.2f units per lag (%s), %.2f per frame (%s) = %.3f / %.3f of the %s bounds"
              % (name, n, "spectra" if itype == 1 else "time series", top[0] * a, top[1], top[2] * b, top[3], top[0], top[2], kind))
        worst = [max(worst[0], top[0]), max(worst[1], top[2])]
    assert worst[0] <= 0.5 and worst[1] <= 0.5, (name, n, worst)
    return worst


POW2 = [16, 64, 256, 1024, 4096]


@pytest.mark.parametrize("n", POW2 + [2, 8, 8192])
def test_radix2_float32_uses_at_most_half_of_the_direct_bounds(n):
    _measure("radix-2 complex64", n, _frames(n) if n <= 4096 else 6, *_radix2(n), "direct")


@pytest.mark.parametrize("n", POW2 + [2, 8, 32768, 65536])
def test_pocketfft_float32_uses_at_most_half_of_the_direct_bounds(n):
    _measure("pocketfft complex64", n, _frames(n) if n <= 4096 else 6, *_pocketfft(), "direct")


def test_pocketfft_float32_at_2_to_the_21_uses_at_most_half_of_the_direct_bounds():
    """(one frame of the two pairs the GPU case runs: a transform of this length takes seconds here)"""
    _measure("pocketfft complex64", 1 << 21, 1, *_pocketfft(), "direct", itypes=[2], only=("mixed x mixed", "mixed x tone_noise"))


@pytest.mark.parametrize("n,radices", [(n, r) for n in (6, 12, 14, 1000, 3840, 6000) for r in MR_PLANS[n]])
def test_mixed_radix_float32_uses_at_most_half_of_its_bounds(n, radices):
    _measure("mixed radix %s" % "x".join(map(str, radices)), n, n + 1 if n <= 14 else 8, *_via_forward(lambda x: _mr_c64(x, radices)), "mixed_radix")


@pytest.mark.parametrize("n", [16000, 20000])
def test_mixed_radix_two_passes_float32_uses_at_most_half_of_its_bounds(n):
    n1, n2, ra, rb = MR_TILE_PLANS[n]
    _measure("mixed radix two passes %d x %d" % (n1, n2), n, 6, *_via_forward(lambda x: _mr_tile_c64(_c64(x), n1, n2, ra, rb)), "mixed_radix_two_passes")


@pytest.mark.parametrize("n", [2 * 2053, 2 * 4099])
def test_chirpz_float32_uses_at_most_half_of_the_chirpz_bounds(n):
    _measure("chirp-z complex64", n, 6, *_via_forward(lambda x: _chirpz_c64(_c64(x), n)), "chirpz")


# ---------------------------------------------------------------------------------------------------------------- planted errors

def _old_and_new(got, n, itype, x0, xs):
    (mag, sc), = xcorr_frames64(n, itype, [x0, xs])
    old = relerr(got.reshape(-1), mag.reshape(-1).astype(np.float32))
    fl, fr = xcorr_bound_check(got, mag, sc, n, itype, "direct", check=False)
    return old, fl, fr


def _noise(n, frames, seed):
    rng = np.random.default_rng(seed)
    return _c64(rng.standard_normal((frames, n)) + 1j * rng.standard_normal((frames, n)))  # what the old tests fed: one amplitude


@pytest.mark.parametrize("n", POW2)
def test_twiddles_rounded_to_16_bits_pass_the_old_metric_and_miss_both_bounds(n):
    """time series (the tables are the transforms'): unit noise against a delayed copy of it plus unit noise -- a peak and a floor"""
    fwd, inv = _radix2(n, bits=16)
    x0 = _noise(n, 12, n)
    xs = _c64(np.roll(x0, n // 5, axis=1) + _noise(n, 12, n + 1))
    got = _xcorr_c64(2, x0, xs, fwd, inv)
    old, fl, fr = _old_and_new(got, n, 2, x0, xs)
    a, b = XCORR_MULT["direct"]
    print("16-bit twiddles n %d: old metric %.2g (passes <= 1e-5); %.1f units per lag (bound %g), %.1f units per frame (bound %g)" % (n, old, fl * a, a, fr * b, b))
    assert old <= TOL_OLD
    assert fl > 1.0 and fr > 1.0, (fl, fr)


@pytest.mark.parametrize("n", POW2)
def test_twiddles_rounded_to_16_bits_miss_both_bounds_on_every_kind(n):
    fwd, inv = _radix2(n, bits=16)
    a, b = XCORR_MULT["direct"]
    frames = _frames(n)
    for i, kind in enumerate(KINDS):
        x0, xs = fft_inputs(kind, n, frames, 7 * n + i), fft_inputs("mixed", n, frames, 7 * n + 4 + i)
        got = _xcorr_c64(2, x0, xs, fwd, inv)
        old, fl, fr = _old_and_new(got, n, 2, x0, xs)
        print("16-bit twiddles n %d %-10s x mixed: %.1f units per lag (bound %g), %.1f units per frame (bound %g); old metric %.2g" % (n, kind, fl * a, a, fr * b, b, old))
        assert fl > 1.0 and fr > 1.0, (kind, fl, fr)


@pytest.mark.parametrize("n", POW2)
def test_one_table_entry_off_by_3e_6_passes_the_old_metric_and_misses_the_per_lag_bound(n):
    """the tone of the bin the entry belongs to against itself (time series), and a unit line in that bin against itself (spectra): the
    product sits in the one bin whose butterflies use the entry"""
    k = n // 8 + 1
    fwd, inv = _radix2(n, off=(k, 3e-6))
    tone = _c64(np.exp(2j * np.pi * k * np.arange(n) / n))[None, :]
    line = np.zeros((1, n), np.complex64)
    line[0, k] = 1.0
    a = XCORR_MULT["direct"][0]
    for itype, x in ((1, line), (2, tone)):
        got = _xcorr_c64(itype, x, x, fwd, inv)
        old, fl, fr = _old_and_new(got, n, itype, x, x)
        print("entry %d of W_%d off by 3e-6, %s: %.1f units per lag (bound %g); old metric %.2g" % (k, n, "spectra" if itype == 1 else "time series", fl * a, a, old))
        assert old <= TOL_OLD
        assert fl > 1.0, fl


@pytest.mark.parametrize("n", POW2)
@pytest.mark.parametrize("itype", ITYPES)
def test_a_wrong_quiet_frame_passes_the_old_metric_and_misses_the_bounds(n, itype):
    """a `mixed` call of three inputs; the quietest live frame of signal 2 zeroed, left unswapped, computed without the conjugate"""
    frames = 33
    ins = [fft_inputs("mixed", n, frames, 31 * n + s) for s in range(3)]
    fwd, inv = _radix2(n)
    (m1, s1), (m2, s2) = xcorr_frames64(n, itype, ins)
    good = [_xcorr_c64(itype, ins[0], ins[s], fwd, inv) for s in (1, 2)]
    T = np.where(s2[0] > 0, s2[0], np.inf)
    f = int(np.argmin(T))
    assert np.isfinite(T[f]) and s2[1][f] < 1e-6 * np.max(s2[1]), "no frame a factor 10^6 under the loudest of its output"
    ref32 = np.concatenate([m1.reshape(-1), m2.reshape(-1)]).astype(np.float32)
    wrong = {"zeroed": np.zeros(n, np.float32),
             "unswapped": _xcorr_c64(itype, ins[0][f:f + 1], ins[2][f:f + 1], fwd, inv, swap=False)[0],
             "no conjugate": _xcorr_c64(itype, ins[0][f:f + 1], ins[2][f:f + 1], fwd, inv, conj=False)[0]}
    assert relerr(np.concatenate([g.reshape(-1) for g in good]), ref32) <= TOL_OLD
    assert max(xcorr_bound_check(good[1], m2, s2, n, itype, check=False)) <= 0.5
    for name, frame in wrong.items():
        bad = good[1].copy()
        bad[f] = frame
        old = relerr(np.concatenate([good[0].reshape(-1), bad.reshape(-1)]), ref32)  # the old tests compare per output; the whole call is no stricter
        old_out = relerr(bad.reshape(-1), m2.reshape(-1).astype(np.float32))
        fl, fr = xcorr_bound_check(bad, m2, s2, n, itype, check=False)
        print("n %d %s frame %d (T %.3g of max %.3g) %s: old metric %.2g per output, %.2g per call (passes <= 1e-5); bounds used %.3g / %.3g times over"
              % (n, "spectra" if itype == 1 else "time series", f, T[f], np.max(s2[0]), name, old_out, old, fl, fr))
        assert old_out <= TOL_OLD and old <= TOL_OLD
        assert fl > 1.0 and fr > 1.0, (name, fl, fr)


def test_multiples_are_under_16():
    for kind, (a, b) in XCORR_MULT.items():
        assert a < 16 and b < 16 and a == int(a) and b == int(b), (kind, a, b)
