"""float64 oracle of clXCorrelate (reference lib/clXCorrelate_impl.cc): magnitudes (:915), the correlation kernel (:851-899) and the
effective max shift (:716-747).  Test infrastructure only."""
import math

import numpy as np


def plan(signal_length, max_search_index):
    """Effective max_shift, or None where the reference exit(1)s."""
    if signal_length % 2 > 0 or max_search_index % 2 > 0:
        return None
    m = max_search_index if max_search_index > 0 else int(0.7 * float(np.float32(signal_length)))
    if max_search_index <= 0 and m % 2 > 0:
        m += 1
    return 1 << max(0, (m - 1).bit_length())


def values(a):
    """The samples the correlation sees: |z| of complex items (as float32, like the block), raw float items."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        re, im = a.real.astype(np.float64), a.imag.astype(np.float64)
        return np.sqrt(re * re + im * im).astype(np.float32).astype(np.float64)
    return a.astype(np.float64)


def curve_literal(x, y, max_shift):
    """Literal restatement of the kernel: one g at a time, the reference's two branches."""
    x, y = values(x), values(y)
    n = len(x)
    out = np.empty(2 * max_shift)
    for g in range(2 * max_shift):
        shift = g - max_shift
        ref_start = shift if shift >= 0 else -shift
        calc_len = n - ref_start
        sxy = sx2 = sy2 = 0.0
        if shift > 0:
            for i in range(calc_len):
                sxy += x[ref_start + i] * y[i]
                sx2 += x[ref_start + i] ** 2
                sy2 += y[i] ** 2
        else:
            for i in range(calc_len):
                sxy += x[i] * y[ref_start + i]
                sx2 += x[i] ** 2
                sy2 += y[ref_start + i] ** 2
        den = sx2 * sy2
        out[g] = sxy / math.sqrt(den) if den != 0.0 else -2.0
    return out


def curve(x, y, max_shift):
    """Vectorised form: float64 FFT correlation for the dot products, cumulative sums (from the start and from the end) for the
    energies over the overlap."""
    x, y = values(x), values(y)
    n = len(x)
    L = 1 << (2 * n).bit_length()
    r = np.fft.irfft(np.fft.rfft(x, L) * np.conj(np.fft.rfft(y, L)), L)  # r[m] = sum_j x[j + m] y[j] (circular, no aliasing)
    shift = np.arange(2 * max_shift) - max_shift
    inside = np.abs(shift) < n
    c = np.where(inside, r[np.where(shift >= 0, shift, L + shift) % L], 0.0)
    pre = lambda v: np.concatenate([[0.0], np.cumsum(v * v)])            # pre[k] = sum_{t < k}
    suf = lambda v: np.concatenate([np.cumsum((v * v)[::-1])[::-1], [0.0]])  # suf[p] = sum_{t >= p}
    px, sx, py, sy = pre(x), suf(x), pre(y), suf(y)
    a = np.clip(np.abs(shift), 0, n)
    ex = np.where(shift >= 0, sx[a], px[n - a])
    ey = np.where(shift >= 0, py[n - a], sy[a])
    den = ex * ey
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(den != 0.0, c / np.sqrt(np.where(den != 0.0, den, 1.0)), -2.0)
    return out


def find_max(cv, max_shift):
    """Maximum and lag (argmax - max_shift); ties to the lowest g, non-finite entries never win."""
    cv = np.asarray(cv)
    fin = np.isfinite(cv)
    if not fin.any():
        return float("nan"), -max_shift
    g = int(np.argmax(np.where(fin, cv, -np.inf)))
    return float(cv[g]), g - max_shift
