"""The yardstick of clFolder, written from the contract in include/mi355_clenabled.h: Python integers for the phase (wrapping modulo
2^64 where the contract says so) and numpy.float32 additions in ascending time, one rounding each.  Slow and plain on purpose."""
import numpy as np

M64 = (1 << 64) - 1


def tri(T):
    T &= M64
    return ((T >> 1) * ((T - 1) & M64) if T % 2 == 0 else T * (((T - 1) & M64) >> 1)) & M64


def phi(model, T):
    phi0, nu, nudot = (int(v) & M64 for v in model)
    T &= M64
    return (phi0 + nu * T + nudot * tri(T)) & M64


def bin_of(model, T, nbin):
    return (((phi(model, T) >> 32) * nbin) >> 32)


def bins(model, T0, n, nbin):
    """bin(T) of T = T0 .. T0 + n - 1 (T wraps modulo 2^64): int32 [n]"""
    return np.array([bin_of(model, T0 + i, nbin) for i in range(n)], np.int32)


def words(phi0, nu, nudot):
    """a model as three uint64 words; nudot may be negative (two's complement)"""
    return np.array([phi0 & M64, nu & M64, nudot & M64], np.uint64)


def fold(x, models, T0, nbin, Ts, tflags=None):
    """x [n][R][F] float32, models [R][3], the absolute index T0 of x[0]: (out [n / Ts][R][nbin][F] float32, hits [n / Ts][R][nbin]
    uint32).  Per (sub-integration, row, bin) the rows that enter are added in ascending T, all channels at once: numpy's float32
    addition is the binary32 addition of the contract, elementwise."""
    x = np.asarray(x, np.float32)
    n, R, F = x.shape
    assert n % Ts == 0
    ns = n // Ts
    out = np.zeros((ns, R, nbin, F), np.float32)
    hits = np.zeros((ns, R, nbin), np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            b = bins(models[r], T0, n, nbin)
            for t in range(n):
                if tflags is not None and tflags[t][r]:
                    continue
                j = t // Ts
                out[j, r, b[t]] = out[j, r, b[t]] + x[t, r]
                hits[j, r, b[t]] += 1
    return out, hits


def pairwise(v):
    """the adjacent-pair tree sum of float32 values, the sum the contract rules out"""
    v = [np.float32(a) for a in v]
    while len(v) > 1:
        v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else np.float32(0)
