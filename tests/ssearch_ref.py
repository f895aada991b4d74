"""The yardstick of clSpectralSearch (include/mi355_clenabled.h, "Spectral search").

Harmonic-sum stage: numpy float32, every addition elementwise in the contract's order -- the accumulator on the left, odd j ascending,
level after level -- so every comparison with the device is array_equal on raw records.  The key order, the record and candidate
layouts and c_h are clPulseSearch's and are imported from tests/psearch_ref.py, not copied.

Spectrum stage: spectrum64 is the definition in float64 (numpy's rfft); spectrum_bound is the per-bin bound the device's float32
spectrum is held to, derived below and never fitted; spectrum32 restates the half-length algorithm of csrc/ssearch.hip in float32
(with faults that can be planted) so that tests/test_ssearch.py can show on the CPU that the bound separates right from wrong.

The bound.  The device transforms z[n] = x[2n] + i x[2n+1] with clFFT at Nb = N / 2 points: Zd[k] = Z[k] + dz[k], and tests/fft_ref.py
holds every component of dz to a u sqrt(L) S_Z with a = FFT_MULT[fft_bound_kind(route)][0], u = 2^-24, L = log2 Nb, S_Z = max |Z| of
the float64 reference: |dz[k]| <= ez = sqrt(2) a u sqrt(L) S_Z.  The untangle is X[k] = A Z[k] + B conj Z[Nb-k] with A = (1 - i t) / 2,
B = (1 + i t) / 2, t = e^(-2 pi i k / N): two Z bins with coefficients of modulus at most 1, so the transform's error reaches X with at
most 2 ez.  The kernel's own roundings are relative to its operands M[k] = |Z[k]| + |Z[Nb-k]| (which is at least |X[k]|; where the two
terms cancel, |X| itself says nothing about the size of the rounding): the four half sums and differences, one rounding each, at most
u M / 2 per component, sqrt(2) u M / 2 for e and as much for d; the twiddle, within one unit in the last place (2 u), two products
and a sum (u each) on |d| <= M / 2, at most 4 sqrt(2) u M / 2; the last addition u |X| <= u M: in all below KERNEL_MULT u M with
KERNEL_MULT = 6.  So
    e[k] = 2 ez + 6 u M[k]
and with w = |X|^2 g, g = inv_sigma^2 / N,
    |dw[k]| <= g (2 |X[k]| e[k] + e[k]^2) + POWER_MULT u w[k],   POWER_MULT = 5
(two squares, their sum, the product with g and g's own rounding: (1 + u)^4 - 1, rounded up to 5 u).  A series of zeros has S_Z = 0
and M = 0: the bound is 0 and the device's w must be exactly 0.  Bins below k_lo are +0 on both sides."""
import numpy as np

import fft_ref
import psearch_ref

PEAK, CAND = psearch_ref.PEAK, psearch_ref.CAND
SERIES, SPECTRUM = 0, 1
MAX_H = 5
KERNEL_MULT, POWER_MULT = 6.0, 5.0
c = psearch_ref.c


def r(k, j, h):
    """the bin of harmonic j of 2^h below bin k: (k j + 2^(h-1)) >> h"""
    return (k * j + (1 << (h - 1))) >> h


def levels(w, H):
    """[s_0, ..., s_H] along the last axis of float32 w, in the contract's order"""
    w = np.asarray(w)
    assert w.dtype == np.float32
    k = np.arange(w.shape[-1], dtype=np.int64)
    s = w.copy()
    out = [s]
    with np.errstate(invalid="ignore", over="ignore"):
        for h in range(1, H + 1):
            for j in range(1, 1 << h, 2):
                s = s + w[..., r(k, j, h)]
            out.append(s)
    assert all(v.dtype == np.float32 for v in out)
    return out


def levels_descending(w, H):
    """odd j descending inside a level: what the contract is NOT"""
    w = np.asarray(w, np.float32)
    k = np.arange(w.shape[-1], dtype=np.int64)
    s = w.copy()
    out = [s]
    for h in range(1, H + 1):
        for j in range((1 << h) - 1, 0, -2):
            s = s + w[..., r(k, j, h)]
        out.append(s)
    return out


def levels_level_first(w, H):
    """a level's new harmonics summed first and added to the running sum afterwards: what the contract is NOT"""
    w = np.asarray(w, np.float32)
    k = np.arange(w.shape[-1], dtype=np.int64)
    s = w.copy()
    out = [s]
    for h in range(1, H + 1):
        t = np.zeros_like(w)
        for j in range(1, 1 << h, 2):
            t = t + w[..., r(k, j, h)]
        s = s + t
        out.append(s)
    return out


def snr(w, H):
    """snr[h][...][k] float32: (s_h - 2^h) c_h, one subtraction and one multiplication"""
    lv = levels(w, H)
    out = np.empty((H + 1,) + lv[0].shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for h, s in enumerate(lv):
            out[h] = (s - np.float32(1 << h)) * c(h)
    return out


def peaks(w, H, Bb):
    """PEAK records [S][Nb / Bb] of w[S][Nb]"""
    w = np.asarray(w, np.float32)
    assert w.ndim == 2 and w.shape[1] % Bb == 0
    S_, Nb = w.shape
    v = snr(w, H).reshape(H + 1, S_, Nb // Bb, Bb)
    hh = np.arange(H + 1, dtype=np.uint32)[:, None, None, None]
    kk = np.arange(Bb, dtype=np.uint32)[None, None, None, :]
    keys = np.where(np.isnan(v), np.uint64(0), psearch_ref.key(v, hh, kk))  # a key of a value is never 0
    best = keys.transpose(1, 2, 0, 3).reshape(S_, Nb // Bb, (H + 1) * Bb).max(axis=2)
    out = np.empty(best.shape, PEAK)
    o = (best >> np.uint64(32)).astype(np.uint32)
    out["snr"] = np.where(o >> np.uint32(31), o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(np.float32)
    out["loc"] = ~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    none = best == 0
    out["snr"][none] = -np.inf
    out["loc"][none] = 0xFFFFFFFF
    return out


def candidates(pk, threshold):
    """the candidate set of PEAK records [S][nblk] as a sorted uint32 array [count][4]: (snr bits, loc, series, block)"""
    return psearch_ref.candidates(np.ascontiguousarray(pk.T), threshold)


def best(pk, Bb):
    """(series, h, k) of the largest record, k the bin in the spectrum: the greatest S/N (+0 above -0), then the smallest h, then the
    smallest k, then the first series"""
    S, nblk = pk.shape
    loc = pk["loc"].astype(np.uint64)
    k = np.arange(nblk, dtype=np.uint64)[None, :] * np.uint64(Bb) + (loc & np.uint64(0xFFFFFF))
    full = ((loc >> np.uint64(24)) << np.uint64(24)) | k  # Nb <= 2^21 < 2^24
    key = (psearch_ref.ordered(pk["snr"]).astype(np.uint64) << np.uint64(32)) | (full ^ np.uint64(0xFFFFFFFF))
    s, b = np.unravel_index(int(np.argmax(key)), pk.shape)
    return int(s), int(pk["loc"][s, b]) >> 24, int(k[s, b])


def pitched(x, pitch, fill=np.nan):
    """x[S][row] -> the flat buffer with rows at `pitch` floats (the last one row long), gaps = fill"""
    return psearch_ref.to_order(np.asarray(x, np.float32), psearch_ref.TRIAL_MAJOR, pitch, fill)


# ---- spectrum stage ----

def gain(inv_sigma, N):
    return np.asarray(inv_sigma, np.float32).astype(np.float64) ** 2 / float(N)


def spectrum64(x, inv_sigma, k_lo):
    """w[S][Nb] float64 of float32 x[S][N]: |rfft|^2 inv_sigma^2 / N without the Nyquist bin, 0 below k_lo"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2
    N = x.shape[1]
    X = np.fft.rfft(x.astype(np.float64), axis=1)[:, :N // 2]
    w = (X.real * X.real + X.imag * X.imag) * gain(inv_sigma, N)[:, None]
    w[:, :k_lo] = 0.0
    return w


def half_transform64(x):
    """Z[S][Nb] complex128: the transform of z[n] = x[2n] + i x[2n+1]"""
    x = np.asarray(x, np.float32).astype(np.float64)
    return np.fft.fft(x[:, 0::2] + 1j * x[:, 1::2], axis=1)


def spectrum_bound(x, inv_sigma, k_lo, kind="direct"):
    """the per-bin bound on |w_device - spectrum64| [S][Nb] (float64), as the module's docstring derives it; kind: fft_bound_kind of the
    internal transform's route"""
    x = np.asarray(x, np.float32)
    N = x.shape[1]
    Nb = N // 2
    Z = half_transform64(x)
    absz = np.abs(Z)
    S_Z = absz.max(axis=1)
    ez = np.sqrt(2.0) * fft_ref.FFT_MULT[kind][0] * fft_ref.fft_unit(Nb) * S_Z
    partner = (Nb - np.arange(Nb)) % Nb
    M = absz + absz[:, partner]
    e = 2.0 * ez[:, None] + KERNEL_MULT * fft_ref.U32 * M
    X = np.fft.rfft(x.astype(np.float64), axis=1)[:, :Nb]
    absx = np.abs(X)
    g = gain(inv_sigma, N)[:, None]
    bound = g * (2.0 * absx * e + e * e) + POWER_MULT * fft_ref.U32 * (absx * absx * g)
    bound[:, :k_lo] = 0.0
    return bound


def spectrum_used(got, x, inv_sigma, k_lo, kind="direct"):
    """the largest used fraction of spectrum_bound over the bins of got[S][Nb] (float32); inf where a bin whose bound is 0 is not
    exactly +0 (bits), or where got is not finite"""
    got = np.asarray(got)
    assert got.dtype == np.float32
    ref, bound = spectrum64(x, inv_sigma, k_lo), spectrum_bound(x, inv_sigma, k_lo, kind)
    assert got.shape == ref.shape
    d = np.abs(got.astype(np.float64) - ref)
    zero = bound == 0
    if not np.all(got.view(np.uint32)[zero] == 0) or not np.isfinite(got).all():
        return float("inf")
    live = ~zero
    return float((d[live] / bound[live]).max()) if live.any() else 0.0


def twiddles(N):
    """(cos, sin)(2 pi k / N) for k <= N / 4 as float32, each from an argument of at most pi / 4 in float64"""
    q = N // 4
    k = np.arange(q + 1)
    low = 2 * k <= q
    a = 2.0 * np.pi * np.where(low, k, q - k) / N
    return np.where(low, np.cos(a), np.sin(a)).astype(np.float32), np.where(low, np.sin(a), np.cos(a)).astype(np.float32)


def spectrum32(x, inv_sigma, k_lo, fault=None):
    """The half-length algorithm in float32, operation by operation as k_ss_power writes it, on a correctly rounded Z (float64
    transform rounded to complex64: within the transform's bound by a wide margin).  fault: None, or one planted error --
    "twiddle_sign" (e^(+2 pi i k / N)), "unconjugated" (Z[Nb-k] taken as it is), "off_by_one" (the partner is Z[Nb-k-1])."""
    x = np.asarray(x, np.float32)
    S, N = x.shape
    Nb = N // 2
    Z = half_transform64(x).astype(np.complex64)
    k = np.arange(Nb)
    partner = ((Nb - k - 1) if fault == "off_by_one" else (Nb - k)) % Nb
    a, b = Z, Z[:, partner]
    ar, ai, br, bi = a.real, a.imag, b.real, b.imag
    if fault == "unconjugated":
        bi = -bi
    cq, sq = twiddles(N)
    fold = np.where(k <= Nb // 2, k, Nb - k)
    cc = np.where(k <= Nb // 2, cq[fold], -cq[fold]).astype(np.float32)
    ss = sq[fold]
    if fault == "twiddle_sign":
        ss = -ss
    h = np.float32(0.5)
    er, ei, dr, di = h * (ar + br), h * (ai - bi), h * (ar - br), h * (ai + bi)
    xr = er + (cc * di - ss * dr)
    xi = ei - (cc * dr + ss * di)
    q = np.asarray(inv_sigma, np.float32)
    g = ((q * q) * np.float32(1.0 / N))[:, None]
    w = (xr * xr + xi * xi) * g
    assert w.dtype == np.float32
    w[:, :k_lo] = 0.0
    return w


def series_cases(N, seed=0):
    """The inputs the spectrum stage is held on, {name: (x[S][N] float32, inv_sigma[S] float32)}:
    tones    S = 3: unit Gaussian noise; noise plus a tone on bin N / 8 + 3; noise plus a tone between two bins (N / 5 + 0.37)
    scaled   S = 2: a series of zeros (inv_sigma 1) and noise scaled by 1e3
    inv_sigma is 1 / the population standard deviation in float64, rounded once, as mi355_psearch_measure gives it"""
    rng = np.random.default_rng(9000 + N % 9973 + seed)
    t = np.arange(N)
    x = rng.standard_normal((3, N))
    x[1] += 0.5 * np.cos(2 * np.pi * (N // 8 + 3) * t / N + 0.3)
    x[2] += 0.5 * np.cos(2 * np.pi * (N // 5 + 0.37) * t / N + 1.1)
    x = x.astype(np.float32)
    y = np.zeros((2, N), np.float32)
    y[1] = (1e3 * rng.standard_normal(N)).astype(np.float32)
    gy = psearch_ref.measure(y, N)[1].astype(np.float32)
    gy[0] = 1.0
    return {"tones": (x, psearch_ref.measure(x, N)[1].astype(np.float32)), "scaled": (y, gy)}


def pulse_train(rng, N, period, amp, phase=0.0):
    """unit Gaussian noise plus one-sample pulses of height amp every `period` samples; float32 [N]"""
    x = rng.standard_normal(N)
    t = np.arange(N)
    x += amp * (((t + 0.5 - phase) % period) < 1.0)
    return x.astype(np.float32)
