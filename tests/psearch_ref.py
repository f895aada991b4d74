"""The yardstick of clPulseSearch: the contract of include/mi355_clenabled.h in numpy float32.

  tree      b_0 = x, b_k[t] = b_(k-1)[t] + b_(k-1)[t + 2^(k-1)]: numpy's float32 addition is IEEE binary32, round to nearest even, one
            rounding per addition, which is what the contract pins
  snr       (b_k[t] - mean 2^k) (inv_sigma c_k), c_k the float32 nearest 2^(-k/2): one float32 subtraction, one float32 multiplication
  key       the 64-bit order of the contract: high word the order-preserving map of the float's bits, low word ~((k << 24) | t)
  peaks     per (block, series) the record of the largest key over the non-NaN snr_k[t]; {-Inf, 0xFFFFFFFF} when there is none
  candidates the set of (snr bits, loc, series, block) of the peaks with snr >= threshold

So every comparison with the device is array_equal on raw records.  Layouts: series-major x[s][t] is what the functions take (s = r D + d);
to_order() makes the buffer of either device order from it."""
import numpy as np

TRIAL_MAJOR, TIME_MAJOR = 0, 1
PEAK = np.dtype([("snr", np.float32), ("loc", np.uint32)])
CAND = np.dtype([("snr", np.float32), ("loc", np.uint32), ("series", np.uint32), ("block", np.uint32)])
C_ODD = np.uint32(0x3F3504F3)  # the float32 nearest 2^(-1/2)


def history(K):
    return (1 << (K - 1)) - 1


def plan(R, D, K):
    """(in_floats_per_sample, history, peaks_per_block)"""
    return R * D, history(K), R * D


def c(k):
    """the float32 nearest 2^(-k/2), as the contract spells it"""
    base = C_ODD.view(np.float32) if k & 1 else np.float32(1.0)
    return np.float32(base * np.float32(2.0 ** -(k // 2)))


def tree(x, K):
    """[b_0, ..., b_(K-1)] along the last axis; b_k is 2^k - 1 samples shorter than x"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    lv = [x]
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, K):
            p, h = lv[-1], 1 << (k - 1)
            lv.append(p[..., :-h] + p[..., h:])
    assert all(b.dtype == np.float32 for b in lv)
    return lv


def snr(x, K, n, mean=None, inv_sigma=None):
    """snr[k][s][t] float32 for t < n; x[s][n + history(K)]"""
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[1] >= n + history(K), "the boxcars read past the input"
    S = x.shape[0]
    mean = np.zeros(S, np.float32) if mean is None else np.asarray(mean, np.float32)
    inv_sigma = np.ones(S, np.float32) if inv_sigma is None else np.asarray(inv_sigma, np.float32)
    out = np.empty((K, S, n), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, b in enumerate(tree(x[:, :n + history(K)], K)):
            m = mean * np.float32(2.0 ** k)
            g = inv_sigma * c(k)
            assert m.dtype == np.float32 and g.dtype == np.float32
            out[k] = (b[:, :n] - m[:, None]) * g[:, None]
    return out


def ordered(v):
    """the order-preserving map of float32 bits to uint32"""
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key(v, k, t):
    loc = (np.asarray(k, np.uint32) << np.uint32(24)) | np.asarray(t, np.uint32)
    return (ordered(v).astype(np.uint64) << np.uint64(32)) | (~loc).astype(np.uint64)


def peaks(x, K, Tb, n, mean=None, inv_sigma=None):
    """PEAK records [n / Tb][S]"""
    assert n % Tb == 0
    s = snr(x, K, n, mean, inv_sigma)  # [K][S][n]
    S, nb = s.shape[1], n // Tb
    s = s.reshape(K, S, nb, Tb)
    kk = np.arange(K, dtype=np.uint32)[:, None, None, None]
    tt = np.arange(Tb, dtype=np.uint32)[None, None, None, :]
    keys = np.where(np.isnan(s), np.uint64(0), key(s, kk, tt))  # a key of a value is never 0
    keys = keys.transpose(2, 1, 0, 3).reshape(nb, S, K * Tb)
    best = keys.max(axis=2)
    out = np.empty((nb, S), PEAK)
    o = (best >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o >> np.uint32(31), o ^ np.uint32(0x80000000), ~o).astype(np.uint32)
    out["snr"] = bits.view(np.float32)
    out["loc"] = ~(best & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    none = best == 0
    out["snr"][none] = -np.inf
    out["loc"][none] = 0xFFFFFFFF
    return out


def peaks_lexicographic(x, K, Tb, n, mean=None, inv_sigma=None):
    """the same records from the rule in words (greatest S/N, +0 above -0, smallest k, smallest t): a plain loop, for tiny cases"""
    s = snr(x, K, n, mean, inv_sigma)
    S, nb = s.shape[1], n // Tb
    out = np.empty((nb, S), PEAK)
    for b in range(nb):
        for i in range(S):
            best = None
            for k in range(K):
                for t in range(Tb):
                    v = s[k, i, b * Tb + t]
                    if np.isnan(v):
                        continue
                    better = best is None or v > best[0] or (v == best[0] and v == 0 and not np.signbit(v) and np.signbit(best[0]))
                    if better:
                        best = (v, k, t)
            out[b, i] = (-np.inf, 0xFFFFFFFF) if best is None else (best[0], (best[1] << 24) | best[2])
    return out


def candidates(pk, threshold):
    """the candidate set of PEAK records [nb][S] as a sorted uint32 array [count][4]: (snr bits, loc, series, block)"""
    nb, S = pk.shape
    with np.errstate(invalid="ignore"):
        b, s = np.nonzero(pk["snr"] >= np.float32(threshold))
    rec = np.stack([pk["snr"][b, s].view(np.uint32), pk["loc"][b, s], s.astype(np.uint32), b.astype(np.uint32)], axis=1).astype(np.uint32)
    return sort_records(rec)


def sort_records(rec):
    """[count][4] uint32 (or a CAND array) in one canonical order"""
    rec = np.ascontiguousarray(rec)
    if rec.dtype == CAND:
        rec = rec.view(np.uint32).reshape(-1, 4)
    rec = rec.reshape(-1, 4)
    return rec[np.lexsort((rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]))]


def to_order(x, order, pitch=None, fill=np.nan):
    """x[s][T] -> the flat device buffer: TIME_MAJOR [t][s]; TRIAL_MAJOR rows of `pitch` floats (the last one T long), gaps = fill"""
    S, T = x.shape
    if order == TIME_MAJOR:
        return np.ascontiguousarray(x.T).reshape(-1)
    p = T if pitch is None else pitch
    assert p >= T
    buf = np.full((S - 1) * p + T, fill, np.float32)
    for s in range(S):
        buf[s * p:s * p + T] = x[s]
    return buf


def sequential(x, k):
    """the left-to-right float32 sum of 2^k neighbours: what the contract is NOT"""
    w = 1 << k
    n = x.shape[-1] - w + 1
    acc = np.zeros(x.shape[:-1] + (n,), np.float32)
    for j in range(w):
        acc = acc + x[..., j:j + n]
    return acc


def measure(x, n):
    """float64 mean and 1 / population standard deviation per series of x[s][:n] (0 where the variance is 0)"""
    v = np.asarray(x, np.float64)[:, :n]
    m = v.mean(axis=1)
    var = ((v - m[:, None]) ** 2).mean(axis=1)
    with np.errstate(divide="ignore"):
        return m, np.where(var == 0, 0.0, 1.0 / np.sqrt(var))


def pulse_scene(seed=2026):
    """The end-to-end fixture: a filterbank x[t][r][f] of unit Gaussian noise, R = 2, F = 64, with a pulse 8 samples wide and `amp` high
    in every channel of row r0, dispersed as trial d0 of a D = 16 table, and the search geometry behind the dedisperser.  With
    inv_sigma = 1 / sqrt(F) the pulse's boxcar of width 8 has S/N 8 F amp c_3 / sqrt(F) = 45 against 32 for widths 4 and 16 and
    39.6 for width 8 one sample off, so the reference puts the global maximum on (r0, d0, k = 3, t0)."""
    import dedisp_ref
    R, F, D, K, Tb, nb = 2, 64, 16, 6, 64, 4
    r0, d0, t0, amp = 1, 11, 150, 2.0
    tab, H = dedisp_ref.delays(1500.0, -300.0 / F, F, 1e-3, np.arange(D) * 4.0)
    n = nb * Tb                  # outputs of the search
    n_dd = n + history(K)        # outputs of the dedisperser
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_dd + H, R, F)).astype(np.float32)
    for f in range(F):
        x[t0 + tab[d0, f]:t0 + tab[d0, f] + 8, r0, f] += np.float32(amp)
    inv_sigma = np.full(R * D, 1.0 / np.sqrt(F), np.float32)
    return dict(R=R, F=F, D=D, K=K, Tb=Tb, nb=nb, H=H, tab=tab, x=x, n=n, n_dd=n_dd, inv_sigma=inv_sigma, r0=r0, d0=d0, t0=t0)
