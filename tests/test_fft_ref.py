"""CPU: the per-frame error bounds of clFFT (tests/fft_ref.py: fft_bound_check against fft_frames64) are fixed here, on float32 transforms
that run on the CPU, and never on a GPU result.

The rule: every CPU float32 evaluation stays at or under HALF of each bound, over the input kinds the GPU tests use (mixed-scale noise
with zero frames, impulses, tones, tone plus noise at -60 dB).  The evaluations are a numpy complex64 radix-2 FFT (_fft2_c64: decimation
in time, one table W_N^k rounded to float, every butterfly in complex64), scipy's complex64 pocketfft where scipy is installed, and, for
the chirp-z routes, a complex64 emulation of their structure (pre-chirp, FFT_m, spectrum product, inverse FFT_m, post-chirp) over the same
radix-2 transform.  In the unit u sqrt(L) S_f they measure at most 1.5 per bin / 1.1 root sum square (direct) and 2.6 / 1.6 (chirp-z);
(a, b) = (4, 3) and (8, 4) keep them under half.  The mixed-radix routes form a butterfly's twiddles W^r as products of one table entry's
squares (more roundings by construction), so they have multiples of their own, fixed by the same rule on complex64 emulations of exactly their
passes and products (_mr_c64, _mr_tile_c64) over the plan of every such length the GPU tests use: at most 6.0 / 3.6 units in one pass,
5.1 / 2.8 in two, hence (13, 8) and (11, 6), the smallest integers at or above twice those figures; with the twiddles read from a table the same passes stay under half of the direct bounds.

Then two planted errors, which the old metric (conftest.relerr <= 1e-5, one scale per call) lets through, must miss the bounds:
the twiddle table rounded to 16 significand bits, and one table entry off by 3e-6 relative.  Every test prints its figures (pytest -s)."""
import numpy as np
import pytest

from conftest import relerr
from fft_ref import FFT_MULT, MR_PLANS, MR_TILE_PLANS, fft_bound_check, fft_frames64, fft_inputs, fft_unit

SIZES = [8, 64, 1024, 4096, 16384, 1000]
KINDS = ["mixed", "impulses", "tones", "tone_noise"]
TOL_OLD = 1e-5


def _frames(n):
    return n if n <= 64 else 24  # short lengths: the identity / one tone per bin; the rest: edges and seeded positions


def _round_bits(t, bits):
    """complex values rounded to `bits` significand bits per component (24 and more: untouched)"""
    if bits >= 24:
        return t
    def rnd(v):
        m, e = np.frexp(v)
        return np.ldexp(np.round(m * 2.0 ** bits) / 2.0 ** bits, e)
    return rnd(t.real) + 1j * rnd(t.imag)


def _table(n, bits=24, off=None):
    """W_n^k = exp(-2 pi i k / n), k < n / 2, in double, rounded to float -- or to `bits` significand bits; off = (k, rel): entry k
    scaled by 1 + rel (the planted errors)"""
    t = np.exp(-2j * np.pi * np.arange(max(n // 2, 1)) / n)
    t = _round_bits(t, bits).astype(np.complex64)
    if off is not None:
        t[off[0]] *= np.complex64(1.0 + off[1])
    return t


def _fft2_c64(x, table, inverse=False):
    """radix-2 decimation-in-time FFT of every row of x in complex64; table = W_n^k, k < n / 2 (conjugated for the inverse, unscaled)"""
    x = np.asarray(x, np.complex64)
    fr, n = x.shape
    lg = n.bit_length() - 1
    assert 1 << lg == n
    rev = np.zeros(n, np.int64)
    for b in range(lg):
        rev |= ((np.arange(n) >> b) & 1) << (lg - 1 - b)
    y = x[:, rev].copy()
    tw = np.conj(table) if inverse else table
    m = 2
    while m <= n:
        h = m // 2
        w = tw[(np.arange(h) * (n // m))]
        y = y.reshape(fr, n // m, 2, h)
        t = (y[:, :, 1, :] * w).astype(np.complex64)
        lo = (y[:, :, 0, :] + t).astype(np.complex64)
        hi = (y[:, :, 0, :] - t).astype(np.complex64)
        y = np.stack([lo, hi], axis=2).reshape(fr, n)
        m *= 2
    assert y.dtype == np.complex64
    return y


def _chirpz_c64(x, n):
    """the chirp-z structure of clFFT in complex64: X[k] = a[k] sum_j (x[j] a[j]) conj(a)[k - j], a[j] = exp(-i pi j^2 / n), as a circular
    convolution of size m = 2^ceil(log2(2n - 1)) (at least 256): tables in double rounded to float, the conjugate chirp's spectrum pre-scaled 1/m"""
    m = 256
    while m < 2 * n - 1:
        m <<= 1
    j = np.arange(n, dtype=np.int64)
    a = np.exp(-1j * np.pi * ((j * j) % (2 * n)) / n)
    b = np.zeros(m, np.complex128)
    b[:n] = np.conj(a)
    b[m - n + 1:] = np.conj(a[1:][::-1])
    bspec = (np.fft.fft(b) / m).astype(np.complex64)
    a32 = a.astype(np.complex64)
    tab = _table(m)
    A = np.zeros((x.shape[0], m), np.complex64)
    A[:, :n] = (np.asarray(x, np.complex64) * a32).astype(np.complex64)
    B = (_fft2_c64(A, tab) * bspec).astype(np.complex64)
    C = _fft2_c64(B, tab, inverse=True)
    return (C[:, :n] * a32).astype(np.complex64)


def _c64(v):
    return np.asarray(v).astype(np.complex64)


def _powers_c64(w1, radix, start=None):
    """k_fft_mr's twiddles of one butterfly: W^r, r < radix, from the table entry W (w1): W^2, W^4, W^8 by squaring, W^r as the product of
    the squares its bits name, lowest first; start: the product begins there (the two-pass form's base entry) instead of at the first square"""
    sq = [w1]
    for q in range(1, 4):
        sq.append(_c64(sq[-1] * sq[-1]) if radix > (1 << q) else sq[-1])
    out = []
    for r in range(radix):
        t = start
        for q in range(4):
            if (r >> q) & 1:
                t = sq[q] if t is None else _c64(t * sq[q])
        out.append(np.ones_like(w1) if t is None else t)
    return out


def _mr_c64(x, radices, products=True, bits=24, off=None):
    """the Stockham passes of k_fft_mr on every row of x in complex64: pass p (radix R, ns = product of the radices before it) takes butterfly
    b = (g, k), k = b mod ns, from x[b + r n / R], multiplies by W_(ns R)^(k r) -- products = True: formed as the kernel forms them, from the
    table entry W_(ns R)^k; False: each read from a table -- and stores the R-point DFT at g ns R + k + s ns.  The planted errors: bits < 24
    rounds every table entry to that many significand bits, off = (k, rel) scales entry k of the last pass' run by 1 + rel"""
    x = _c64(x)
    n = x.shape[1]
    ns = 1
    for R in radices:
        nb = n // R
        b = np.arange(nb)
        k, g = b % ns, b // ns
        v = np.stack([x[:, b + r * nb] for r in range(R)], axis=2)  # (frames, butterflies, R)
        if ns > 1:
            if products:
                run = _c64(_round_bits(np.exp(-2j * np.pi * np.arange(ns) / (ns * R)), bits))
                if off is not None and ns * R == n:
                    run[off[0]] *= np.complex64(1.0 + off[1])
                tw = np.stack(_powers_c64(run[k], R), axis=1)
            else:
                tw = _c64(np.exp(-2j * np.pi * np.outer(k, np.arange(R)) / (ns * R)))
            v = _c64(v * tw)
        D = _c64(np.exp(-2j * np.pi * np.outer(np.arange(R), np.arange(R)) / R))
        V = _c64(v[:, :, :1] * D[0])
        for r in range(1, R):  # (the R-point DFT as a plain complex64 sum: elementwise operations only, the same on every machine)
            V = _c64(V + _c64(v[:, :, r:r + 1] * D[r]))
        y = np.empty_like(x)
        for s_ in range(R):
            y[:, g * ns * R + k + s_ * ns] = V[:, :, s_]
        x, ns = y, ns * R
    return x


def _mr_tile_c64(x, n1, n2, ra, rb):
    """the two passes of k_fft_mr_tile in complex64: x as n1 rows of n2; pass A: every column by the passes ra, times W_N^(n2 k1) formed from the
    table entries W_N^(n2 k) and W_N^(n2 ns) (k1 = k + r ns, ns = n1 / the last radix of ra) as in _powers_c64; pass B: every column k1 of the
    n2 x n1 workspace by the passes rb; X[k1 + n1 k2]"""
    fr, n = x.shape
    cols = _c64(x).reshape(fr, n1, n2).transpose(0, 2, 1).reshape(fr * n2, n1)
    A = _mr_c64(cols, ra).reshape(fr, n2, n1)
    R = ra[-1]
    ns = n1 // R
    twn = _c64(np.exp(-2j * np.pi * np.arange(n) / n))
    k1 = np.arange(n1)
    i2 = np.arange(n2)[:, None]
    base = twn[i2 * (k1 % ns)[None, :]]
    pw = _powers_c64(twn[i2 * ns], R, start=1)  # (n2, 1) each; start = 1: the powers as factors of the base
    t = base
    for q in range(4):
        sel = ((k1 // ns) >> q) & 1 == 1
        sq = pw[1 << q] if (1 << q) < R else None
        if sq is not None and sel.any():
            t = np.where(sel[None, :], _c64(t * sq), t)
    A = _c64(A * t)
    rows = A.transpose(0, 2, 1).reshape(fr * n1, n2)
    return _mr_c64(rows, rb).reshape(fr, n1, n2).transpose(0, 2, 1).reshape(fr, n)


def _used(got, x, n, kind="direct"):
    return fft_bound_check(got, fft_frames64(n, True, None, False, x), n, kind, check=False)


def _inputs(n):
    return {k: fft_inputs(k, n, _frames(n), 10 * n + i) for i, k in enumerate(KINDS)}


def test_the_new_per_bin_bound_is_never_looser_than_the_old_one():
    """S_f <= the call's max |ref|, and a u sqrt(L) <= 1e-5 for every length clFFT takes: a result inside the per-bin bound is inside
    relerr <= 1e-5"""
    for kind, (a, b) in FFT_MULT.items():
        for n in (2, 8, 4096, 1 << 24, 8388608 - 1):
            print("%s n %d: a u sqrt(L) = %.3g" % (kind, n, a * fft_unit(n)))
            assert a * fft_unit(n) * np.sqrt(2.0) <= TOL_OLD  # sqrt 2: per component against relerr's modulus
    assert abs(4 * fft_unit(8) - 4.1e-7) < 1e-8 and abs(4 * fft_unit(4096) - 8.3e-7) < 1e-8 and abs(4 * fft_unit(1 << 24) - 1.2e-6) < 5e-8
    x = fft_inputs("mixed", 64, 9, 1)
    ref = fft_frames64(64, True, None, False, x)
    assert np.abs(ref).max(axis=1).max() == np.abs(ref).max()


@pytest.mark.parametrize("n", [s for s in SIZES if s & (s - 1) == 0])
def test_radix2_float32_uses_at_most_half_of_the_direct_bounds(n):
    tab = _table(n)
    for kind, x in _inputs(n).items():
        fb, fr = _used(_fft2_c64(x, tab), x, n)
        print("radix-2 complex64 n %d %-10s used %.3f (bin) %.3f (rss) of the direct bounds" % (n, kind, fb, fr))
        assert fb <= 0.5 and fr <= 0.5, (kind, fb, fr)
    w = np.blackman(n).astype(np.float32)
    x = fft_inputs("mixed", n, _frames(n), n + 5)
    got = _fft2_c64((x * w).astype(np.complex64), tab)
    fb, fr = fft_bound_check(got, fft_frames64(n, True, w, False, x), n, "direct", check=False)
    print("radix-2 complex64 n %d windowed   used %.3f (bin) %.3f (rss)" % (n, fb, fr))
    assert fb <= 0.5 and fr <= 0.5


@pytest.mark.parametrize("n", SIZES + [12000])
def test_pocketfft_float32_uses_at_most_half_of_the_direct_bounds(n):
    sfft = pytest.importorskip("scipy.fft")
    for kind, x in _inputs(n).items():
        got = sfft.fft(x, axis=1)
        assert got.dtype == np.complex64
        fb, fr = _used(got, x, n)
        print("pocketfft complex64 n %d %-10s used %.3f (bin) %.3f (rss) of the direct bounds" % (n, kind, fb, fr))
        assert fb <= 0.5 and fr <= 0.5, (kind, fb, fr)


@pytest.mark.parametrize("n", [12, 1000, 1200, 4099, 16385])
def test_chirpz_float32_uses_at_most_half_of_the_chirpz_bounds(n):
    for kind, x in _inputs(n).items():
        x = x[:12]
        fb, fr = _used(_chirpz_c64(x, n), x, n, "chirpz")
        print("chirp-z complex64 n %d %-10s used %.3f (bin) %.3f (rss) of the chirp-z bounds" % (n, kind, fb, fr))
        assert fb <= 0.5 and fr <= 0.5, (kind, fb, fr)


@pytest.mark.parametrize("n", [s for s in SIZES if s & (s - 1) == 0])
def test_twiddles_rounded_to_16_bits_miss_both_bounds(n):
    tab = _table(n, bits=16)
    for kind, x in _inputs(n).items():
        a, b = FFT_MULT["direct"]
        fb, fr = _used(_fft2_c64(x, tab), x, n)
        print("16-bit twiddles n %d %-10s: %.1f units per bin (bound %g), %.1f units rss (bound %g)" % (n, kind, fb * a, a, fr * b, b))
        assert fb > 1.0 and fr > 1.0, (kind, fb, fr)


def test_twiddles_rounded_to_16_bits_pass_the_old_metric():
    n = 64
    tab = _table(n, bits=16)
    rng = np.random.default_rng(64)
    x = (rng.standard_normal((37, n)) + 1j * rng.standard_normal((37, n))).astype(np.complex64)  # what the old tests fed: one amplitude
    t = fft_inputs("tones", n, n, 3)
    for name, v in (("noise", x), ("tones", t)):
        got, ref = _fft2_c64(v, tab), fft_frames64(n, True, None, False, v)
        old = relerr(got.reshape(-1), ref.reshape(-1))
        fb, fr = fft_bound_check(got, ref, n, "direct", check=False)
        print("16-bit twiddles n %d %s: old metric %.2g (passes <= 1e-5); new bounds used %.1f / %.1f times over" % (n, name, old, fb, fr))
        assert old <= TOL_OLD and fb > 1.0 and fr > 1.0


@pytest.mark.parametrize("n", [s for s in SIZES if s & (s - 1) == 0])
def test_one_table_entry_off_by_3e_6_misses_the_per_bin_bound_on_impulses(n):
    k = max(1, n // 8 + 1) if n > 8 else 1
    tab = _table(n, off=(k, 3e-6))
    x = fft_inputs("impulses", n, n if n <= 1024 else 64, n)
    a = FFT_MULT["direct"][0]
    got, ref = _fft2_c64(x, tab), fft_frames64(n, True, None, False, x)
    fb, fr = fft_bound_check(got, ref, n, "direct", check=False)
    old = relerr(got.reshape(-1), ref.reshape(-1))
    print("entry %d of W_%d off by 3e-6: %.1f units per bin (bound %g); old metric %.2g" % (k, n, fb * a, a, old))
    assert fb > 1.0
    assert old <= TOL_OLD  # and the old metric lets it through at every length, 4096 among them


@pytest.mark.parametrize("n,radices", [(n, r) for n, plans in MR_PLANS.items() for r in plans])
def test_mixed_radix_float32_uses_at_most_half_of_its_bounds(n, radices):
    """the pass structure of k_fft_mr with its twiddle products: held to half of the mixed-radix multiples; with every twiddle read from a
    table the same passes stay under half of the DIRECT bounds -- the products are what the route's own multiples pay for"""
    a, b = FFT_MULT["mixed_radix"]
    for kind, x in _inputs(n).items():
        ref = fft_frames64(n, True, None, False, x)
        fb, fr = fft_bound_check(_mr_c64(x, radices), ref, n, "mixed_radix", check=False)
        tb, tr = fft_bound_check(_mr_c64(x, radices, products=False), ref, n, "direct", check=False)
        print("mixed radix %s n %d %-10s: %.2f units per bin, %.2f rss = %.3f / %.3f of its bounds; twiddles from a table: %.3f / %.3f of the direct bounds"
              % ("x".join(map(str, radices)), n, kind, fb * a, fr * b, fb, fr, tb, tr))
        assert fb <= 0.5 and fr <= 0.5, (kind, fb, fr)
        assert tb <= 0.5 and tr <= 0.5, (kind, tb, tr)


@pytest.mark.parametrize("n", list(MR_TILE_PLANS))
def test_mixed_radix_two_passes_float32_uses_at_most_half_of_its_bounds(n):
    n1, n2, ra, rb = MR_TILE_PLANS[n]
    a, b = FFT_MULT["mixed_radix_two_passes"]
    for i, kind in enumerate(KINDS):
        x = fft_inputs(kind, n, 24 if n < 100000 else 2, 3 * n + i)
        fb, fr = fft_bound_check(_mr_tile_c64(x, n1, n2, ra, rb), fft_frames64(n, True, None, False, x), n, "mixed_radix_two_passes", check=False)
        print("mixed radix two passes %d x %d n %d %-10s: %.2f units per bin, %.2f rss = %.3f / %.3f of its bounds" % (n1, n2, n, kind, fb * a, fr * b, fb, fr))
        assert fb <= 0.5 and fr <= 0.5, (kind, fb, fr)


def test_planted_errors_miss_the_bounds_at_1000_points():
    """the length of the list that is no power of two, on the structure it runs (k_fft_mr 10x10x10, twiddle products, the mixed-radix multiples):
    table entries rounded to 16 bits miss both bounds on every input kind, one entry of the last pass' run off by 3e-6 misses the per-bin bound
    on the impulse set (the kernel raises the entry to powers up to 9, so here the old metric sees it too: its figure is printed, not asserted)"""
    n, radices = 1000, MR_PLANS[1000][0]
    a, b = FFT_MULT["mixed_radix"]
    for kind, x in _inputs(n).items():
        fb, fr = fft_bound_check(_mr_c64(x, radices, bits=16), fft_frames64(n, True, None, False, x), n, "mixed_radix", check=False)
        print("16-bit twiddles n %d %-10s: %.1f units per bin (bound %g), %.1f units rss (bound %g)" % (n, kind, fb * a, a, fr * b, b))
        assert fb > 1.0 and fr > 1.0, (kind, fb, fr)
    x = fft_inputs("impulses", n, n, n)
    got, ref = _mr_c64(x, radices, off=(13, 3e-6)), fft_frames64(n, True, None, False, x)
    fb, fr = fft_bound_check(got, ref, n, "mixed_radix", check=False)
    print("entry 13 of the last run of W_%d off by 3e-6: %.1f units per bin (bound %g); old metric %.2g"
          % (n, fb * a, a, relerr(got.reshape(-1), ref.reshape(-1))))
    assert fb > 1.0
