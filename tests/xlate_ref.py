"""Yardstick for clFreqXlatingFIRFilter: plain numpy, float64 (the contract is in include/mi355_clenabled.h).

Form 1 (what the block computes): band-pass taps, decimate, rotate by an integer phase
    y_c[m] = r(m) s[m],   s[m] = sum_k b[k] x[m D - k],   r(m) = exp(-j 2 pi P(m) / 2^64),   P(m) = (phase + inc m) mod 2^64
with in[K-1] = x[0] (history-prefixed).  On the GPU the yardstick takes b from get_bandpass_taps() and (phase, inc) from get_state(), so
library-versus-numpy sincos and double-rounding differences cannot enter the value comparison; b and inc are checked on their own
(check_bandpass, check_inc).  The phase is evaluated in Python integers.

Form 2 (independent): mix x down by the exact f / fs, filter with h, decimate.  It pins the sign conventions (test_xlate.py).

Tolerance, per output and per component, u = 2^-24:
    bound = 2 B + 8 u (|Re s| + |Im s|),   B = 2 (2 K + 2) u sum_k (|Re b| + |Im b|) max(|Re x|, |Im x|) over the window
B is resampler_ref.bound's form with n_eff = 2 K: a complex dot product has 2 K products per component, and n_eff u sum |a||b| bounds a
float32 sum of them in any order, with or without FMA; + 2 for the final roundings, times 2 for everything second-order.  So every
component of the float sum s~ is within B of s.  The output is fl(r~ s~): r~ is the double phasor rounded to float (u relative per
component), and each output component is two products and one sum, at most three more roundings, so
    |Re y~ - Re y| <= B (|Re r| + |Im r|) + 4 u (|Re s| + |Im s|) (1 + O(u)) <= sqrt(2) B + 4 u (...) (1 + O(u)),
the same for Im.  2 B and 8 u leave sqrt(2) and 2 in hand."""
import numpy as np

U = 2.0 ** -24
TWO64 = 1 << 64


def f32c(a):
    return np.asarray(a).astype(np.complex64)


def round_taps(h):
    """taps rounded to float32 (complex64 when complex), returned in float64 / complex128"""
    h = np.asarray(h).reshape(-1)
    return h.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(h) else h.astype(np.float32).astype(np.float64)


def make_taps(K, complex_taps, seed):
    """seeded standard normal, not a designed low-pass: a wrong index shows at full scale"""
    rng = np.random.default_rng(seed)
    if complex_taps:
        return (rng.standard_normal(K) + 1j * rng.standard_normal(K)).astype(np.complex64)
    return rng.standard_normal(K).astype(np.float32)


def make_input(n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def plan(D, K, n):
    """items of history-prefixed input a call of n outputs reads"""
    return 0 if n == 0 else n * D + K - 1


def frac(v):
    return v - np.floor(v)


def inc_of(f, D, fs):
    """round(frac(f D / fs) 2^64) mod 2^64 as a Python integer, from the signed fraction nearest zero (a small negative frequency keeps
    its precision, and -f gives exactly the negated increment)"""
    t = f * D / fs
    t -= float(np.round(t))
    return int(round(t * 2.0 ** 64)) % TWO64


def bandpass64(h, f, fs):
    """h[k] exp(+j 2 pi frac(k f / fs)) in float64, h rounded to float32 first"""
    h = round_taps(h)
    k = np.arange(h.size, dtype=np.float64)
    return h * np.exp(2j * np.pi * frac(k * (f / fs)))


def check_bandpass(b, h, f, fs):
    """|b[k] - h[k] exp(j 2 pi frac(k f / fs))| <= 2^-23 |h[k]| per component"""
    want = bandpass64(h, f, fs)
    b = np.asarray(b).astype(np.complex128)
    lim = 2.0 ** -23 * np.abs(round_taps(h))
    return bool(np.all(np.abs(b.real - want.real) <= lim) and np.all(np.abs(b.imag - want.imag) <= lim))


def check_inc(inc, f, D, fs):
    """inc 2^-64 within 2^-52 (wrapped) of frac(f D / fs)"""
    d = inc / 2.0 ** 64 - float(frac(f * D / fs))
    d -= round(d)
    return abs(d) <= 2.0 ** -52


def windows(a, D, K, n):
    """(n, K) view: row m is a[m D .. m D + K)"""
    return np.lib.stride_tricks.sliding_window_view(a, K)[::D][:n]


def fir_sums(b, in_hist, D, n):
    """s[m] = sum_k b[k] in[m D + K - 1 - k] in float64; `in_hist` rounded to float32 first"""
    b = np.asarray(b).astype(np.complex128)
    x = f32c(in_hist).astype(np.complex128)
    return windows(x, D, b.size, n) @ b[::-1]


def phasor(phase, inc, n):
    """exp(-j 2 pi P(m) / 2^64), P(m) = (phase + inc m) mod 2^64 in Python integers, as a signed fraction of a turn"""
    out = np.empty(n, np.complex128)
    for m in range(n):
        p = (int(phase) + int(inc) * m) % TWO64
        if p >= TWO64 // 2:
            p -= TWO64
        out[m] = np.exp(-1j * np.pi * (p / 2.0 ** 63))
    return out


def xlate(b, in_hist, D, n, phase, inc):
    """form 1: (y, s)"""
    s = fir_sums(b, in_hist, D, n)
    return phasor(phase, inc, n) * s, s


def xlate_mix(h, f, fs, in_hist, D, n):
    """form 2: mix down by the exact f / fs (x[t] exp(-j 2 pi f t / fs), t = 0 at in[K-1]), filter with h, decimate"""
    h = round_taps(h).astype(np.complex128)
    x = f32c(in_hist).astype(np.complex128)
    t = np.arange(x.size, dtype=np.float64) - (h.size - 1)
    mixed = x * np.exp(-2j * np.pi * frac(t * (f / fs)))
    return windows(mixed, D, h.size, n) @ h[::-1]


def bound(b, in_hist, D, n, s):
    b = np.asarray(b).astype(np.complex128)
    K = b.size
    x = f32c(in_hist).astype(np.complex128)
    mag = np.maximum(np.abs(x.real), np.abs(x.imag))
    absb = np.abs(b.real) + np.abs(b.imag)
    B = 2.0 * (2 * K + 2) * U * (windows(mag, D, K, n) @ absb[::-1])
    return 2.0 * B + 8.0 * U * (np.abs(s.real) + np.abs(s.imag))


def worst(got, want, bnd):
    """largest error / bound over all components (NaN counts as infinite; a bound of 0 with an error of 0 counts as 0)"""
    got = np.asarray(got).astype(np.complex128)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(r.max()) if r.size else 0.0
