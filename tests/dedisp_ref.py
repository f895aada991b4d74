"""The yardstick of clDedisperser: the contract of include/mi355_clenabled.h in numpy.  One float32 accumulator array per (row, trial),
a loop over the channels in ascending order, `acc = acc + x[t + delay]` -- numpy's float32 addition is IEEE binary32, round to nearest
even, one rounding per addition, which is exactly what the contract pins -- and every channel whose entry is -1 skipped.  So every
comparison with the device is array_equal.

Layouts: x[t][r][f] float32, delay[d][f] int32 (0 .. H or -1), TIME_MAJOR y[t][r][d], TRIAL_MAJOR y[r][d][t].

delays(): the formula of mi355_dedisp_delays in numpy float64, operation by operation in the order of the contract."""
import numpy as np

TRIAL_MAJOR, TIME_MAJOR = 0, 1
KDM = 4.148808e3


def dedisperse(x, delay, n, order=TIME_MAJOR):
    """y for the first n output samples; x holds at least n + max(delay) samples"""
    x = np.asarray(x)
    delay = np.asarray(delay)
    assert x.dtype == np.float32 and x.ndim == 3 and delay.ndim == 2 and delay.shape[1] == x.shape[2]
    assert delay.min(initial=0) >= -1 and n + int(delay.max(initial=0)) <= x.shape[0], "the table reads past the input"
    T, R, F = x.shape
    D = delay.shape[0]
    acc = np.zeros((R, D, n), np.float32)  # +0.0
    for f in range(F):
        for d in range(D):
            k = int(delay[d, f])
            if k < 0:
                continue
            acc[:, d, :] = acc[:, d, :] + x[k:k + n, :, f].T
    assert acc.dtype == np.float32
    return acc if order == TRIAL_MAJOR else np.ascontiguousarray(acc.transpose(2, 0, 1))


def delays(f0_mhz, df_mhz, F, tsamp_s, dm, exact=False):
    """(delay[d][f] int32, max) -- or, with exact=True, the float64 values before rounding"""
    f = np.arange(F, dtype=np.float64)
    nu = np.float64(f0_mhz) + f * np.float64(df_mhz)
    assert np.all(nu > 0) and tsamp_s > 0
    ref = nu.max()
    inv = 1.0 / (nu * nu)
    inv_ref = 1.0 / (ref * ref)
    dm = np.asarray(dm, np.float64).reshape(-1)
    assert np.all(dm >= 0) and np.all(np.isfinite(dm))
    k = KDM * dm
    v = (k[:, None] * (inv - inv_ref)[None, :]) / np.float64(tsamp_s)
    if exact:
        return v
    out = np.rint(v).astype(np.int64)
    assert out.min() >= 0 and out.max() <= 1 << 20
    return out.astype(np.int32), int(out.max())


def plan(R, F, D, H):
    """(in_floats_per_sample, history, out_floats_per_sample)"""
    return R * F, H, R * D


def gaussian(rng, T, R, F):
    """seeded signed Gaussian float32: a wrong summation order shows in the bits"""
    return rng.standard_normal((T, R, F)).astype(np.float32)


def random_table(rng, D, F, H, kill=0.0):
    """seeded non-monotone table with entries anywhere in 0 .. H; `kill`: share of -1 entries"""
    t = rng.integers(0, H + 1, size=(D, F)).astype(np.int32)
    if kill:
        t[rng.random((D, F)) < kill] = -1
    return t


def smooth_table(rng, D, F, H, wobble=2):
    """a table whose entries move slowly with trial and channel (what the tiled route is for), with a seeded wobble"""
    d = np.arange(D)[:, None] / max(D - 1, 1)
    f = (F - 1 - np.arange(F))[None, :] / max(F - 1, 1)
    t = np.rint(d * f * max(H - wobble, 0)).astype(np.int64) + rng.integers(0, wobble + 1, size=(D, F))
    return np.clip(t, 0, H).astype(np.int32)
