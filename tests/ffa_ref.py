"""The yardstick of clPeriodSearch (include/mi355_clenabled.h, "Period search"): numpy float32, the recursion exactly as the contract
writes it, stage by stage; shift(L, i, r) in Python integers; the evaluation with the key order built from integer keys."""
import numpy as np

PEAK = np.dtype([("snr", np.float32), ("loc", np.uint32)])
EMPTY_KEY = 0x007FFFFF00000000  # decodes to {-Inf, 0xFFFFFFFF}: below the key of every value


def shift(L, i, r):
    """sh(i, r) = sum over stages sg = 1 .. L of bit_(sg-1)(r) (((i >> (L - sg)) + 1) >> 1)"""
    return sum(((r >> (sg - 1)) & 1) * (((i >> (L - sg)) + 1) >> 1) for sg in range(1, L + 1))


def transform(rows):
    """rows: float32 [m][p], m = 2^L -> the profiles y [m][p] (one binary32 addition per value and stage, head on the left)"""
    a = np.array(rows, np.float32)
    m, p = a.shape
    L = m.bit_length() - 1
    assert m == 1 << L and L >= 1
    j = np.arange(p)
    with np.errstate(all="ignore"):
        for sg in range(1, L + 1):
            g, h = 1 << sg, 1 << (sg - 1)
            grp = a.reshape(m // g, g, p)  # every group of g rows at once: the same additions, element by element
            out = np.empty_like(grp)
            for i in range(g):
                out[:, i] = grp[:, i >> 1] + grp[:, h + (i >> 1)][:, (j + ((i + 1) >> 1)) % p]
            a = out.reshape(m, p)
    return a


def c(e):
    """the binary32 nearest 2^(-e/2), as clPulseSearch writes it"""
    return np.array([(0x3F3504F3 if e & 1 else 0x3F800000) - ((e >> 1) << 23)], np.uint32).view(np.float32)[0]


def keys(y, L, K, mean, inv_sigma):
    """y: float32 [m][p] -> uint64 [m], the largest key of every profile (EMPTY_KEY where no value is not NaN)"""
    y = np.asarray(y, np.float32)
    m, p = y.shape
    mean, inv_sigma = np.float32(mean), np.float32(inv_sigma)
    j = np.arange(p)
    best = np.full(m, EMPTY_KEY, np.uint64)
    b = y.copy()
    with np.errstate(all="ignore"):
        for k in range(K):
            if k:
                b = b + b[:, (j + (1 << (k - 1))) % p]
            snr = (b - mean * np.float32(1 << (L + k))) * (inv_sigma * c(L + k))
            u = snr.view(np.uint32).astype(np.uint64)
            o = np.where(u >> np.uint64(31), u ^ np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
            loc = np.uint64(k << 24) | j.astype(np.uint64)
            key = (o << np.uint64(32)) | (loc ^ np.uint64(0xFFFFFFFF))[None, :]
            key = np.where(np.isnan(snr), np.uint64(0), key)
            best = np.maximum(best, key.max(axis=1))
    return best


def records(key):
    """uint64 keys -> PEAK records"""
    key = np.asarray(key, np.uint64)
    o = (key >> np.uint64(32)).astype(np.uint32)
    out = np.empty(key.shape, PEAK)
    out["snr"] = np.where(o & np.uint32(0x80000000), o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(np.float32)
    out["loc"] = ~(key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return out


def search(x, S, p_lo, p_hi, L, K, mean=None, inv_sigma=None, in_pitch=None, prefill=np.nan, profiles=None):
    """x: float32, x[s in_pitch + t] -> (peaks PEAK [S][P][m], profiles float32 [S][P][m][p_hi] with `prefill` where j >= p).
    `profiles`: the profiles of an earlier search of the same input (other statistics), taken instead of transforming again"""
    m, P = 1 << L, p_hi - p_lo + 1
    N = m * p_hi
    pitch = N if in_pitch is None else in_pitch
    x = np.asarray(x, np.float32).reshape(-1)
    mean = np.zeros(S, np.float32) if mean is None else np.asarray(mean, np.float32)
    inv_sigma = np.ones(S, np.float32) if inv_sigma is None else np.asarray(inv_sigma, np.float32)
    peaks = np.empty((S, P, m), PEAK)
    prof = np.full((S, P, m, p_hi), prefill, np.float32)
    for s in range(S):
        for pi in range(P):
            p = p_lo + pi
            y = transform(x[s * pitch:s * pitch + m * p].reshape(m, p)) if profiles is None else profiles[s, pi, :, :p]
            prof[s, pi, :, :p] = y
            peaks[s, pi] = records(keys(y, L, K, mean[s], inv_sigma[s]))
    return peaks, prof


def best(peaks):
    """(s, pi, i) of the largest record: the greatest S/N (+0 above -0), then the smallest loc, then the first in the array's order"""
    u = peaks["snr"].view(np.uint32).astype(np.uint64)
    o = np.where(u >> np.uint64(31), u ^ np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    key = (o << np.uint64(32)) | (peaks["loc"].astype(np.uint64) ^ np.uint64(0xFFFFFFFF))
    return np.unravel_index(int(np.argmax(key)), peaks.shape)


def pulsar(rng, n, period, width, height, mean=10.0, sigma=2.0, phase=0.0):
    """Gaussian noise (mean, sigma) plus a `height`-high pulse of `width` samples every `period` samples, pulse c beginning at the
    sample nearest phase + c period; float32 [n]"""
    x = rng.normal(mean, sigma, n)
    t = np.arange(n)
    x += height * (((t + 0.5 - phase) % period) < width)
    return x.astype(np.float32)
