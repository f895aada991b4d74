"""The yardstick of clPolyphaseChannelizer: plain numpy, float64.  Plain module (no fixtures), shared by tests/test_fir_ref.py (CPU),
tests/test_pfb_window_gpu.py and the channelizer cases of tests/switch_cases.py.

Contract (include/mi355_clenabled.h): taps h[0..K), M channels, R new items per step, `x_hist` the history-prefixed input
of nsteps R - R + K items.  Step i reads the items [i R, i R + K) of it:

    u_i[c] = sum_k h[k] x_hist[i R + K-1-k] exp(+2 pi j c (k + i (M - R)) / M)             out[i nmap + q] = u_i[ch_map[q]]

evaluated here as the branch sums z_i[j] = sum_p h[j + M p] x_hist[i R + K-1 - j - M p] (arm j, P = ceil(K / M) taps at most), an M-point
backward DFT over j, and the rotation exp(2 pi j c i (M - R) / M) of an oversampled bank.

The tolerance (`bound`), per step, the same for every channel and component of it: the model of tests/fengine_ref.py -- branch-filter errors
carried through the M-point DFT plus the transform's own error, root-sum-square,

    sigma_i = u Q_i sqrt(9 ceil(log2 M) + P + 2),     Q_i^2 = sum_j a_i[j]^2,  a_i[j] = sum_p |h[j + M p]| |x_hist[...]|,     bound = 8 sigma_i

-- extended to R != M: the window of step i starts at i R instead of i M, and the rotation is the one spare operation the model already counts
(on the kernels it is an index rotation of the branch outputs or an exact quarter turn).  Everything in it comes from taps and samples.
"""
import numpy as np

from fengine_ref import K_SIGMA, U

PMAXR_CAP = 32


def pmaxr(P):
    """rows of M items a non-finite item may reach (include/mi355_clenabled.h): the kernels round the taps per arm up with zeros -- to 8, 16
    or 32 up to 32 taps per arm (PMAXR = 32), to 64 on the power-of-two kernels up to 64, to the next multiple of 16 beyond"""
    return 32 if P <= 32 else 64 if P <= 64 else (P + 15) // 16 * 16


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def make_taps(M, P, seed=0):
    """P taps per arm, the last arm ragged where P is odd and above 1; seeded standard normal over sqrt(P), NOT a designed low-pass, no exact zero"""
    K = M * P - (M // 3 if P % 2 and P > 1 else 0)
    h = (np.random.default_rng(5000 + 13 * M + P + seed).standard_normal(K) / np.sqrt(P)).astype(np.float32)
    assert np.all(h != 0)
    return h


def ninput(K, R, nsteps):
    return nsteps * R - R + K


def make_input(K, R, nsteps, seed=0):
    return crandn(np.random.default_rng(191 + seed), ninput(K, R, nsteps))


def maps(M):
    """the channel maps of a case: the identity, and one that repeats and omits channels (16 or more entries where the bank has them)"""
    ident = list(range(M))
    if M <= 3:
        return ident, [M - 1, 0, 0]
    return ident, [M - 1, 0] + [(3 * q + 1) % M for q in range(M // 2 + 1)] + [0]


_BLOCK = 32


def _branches(h, x, M, R, i0, n):
    """(z[n][M] complex128, a[n][M]) of steps i0 .. i0 + n - 1"""
    K = h.size
    P = -(-K // M)
    hp = np.zeros(P * M)
    hp[:K] = h
    k = np.arange(P * M, dtype=np.int64)
    idx = ((i0 + np.arange(n, dtype=np.int64)) * R + K - 1)[:, None] - k[None, :]
    live = idx >= 0                                   # (only the zero padding of the last arm reaches in front of the buffer)
    xs = np.where(live, x[np.where(live, idx, 0)], 0.0)
    seg = xs * hp[None, :]
    z = seg.reshape(n, P, M).sum(axis=1)
    a = (np.abs(np.nan_to_num(xs, nan=0.0, posinf=0.0, neginf=0.0)) * np.abs(hp)[None, :]).reshape(n, P, M).sum(axis=1)
    return z, a


def channelize(h, M, R, ch_map, x_hist, nsteps):
    """(out complex128 [nsteps * nmap], bound float64 [nsteps]): the formula above and the tolerance of every component of a step"""
    h = np.asarray(h, np.float32).astype(np.float64)
    x = np.asarray(x_hist).astype(np.complex64).astype(np.complex128)
    K = h.size
    assert x.size >= ninput(K, R, nsteps)
    P = -(-K // M)
    cm = np.asarray(ch_map, np.int64)
    out = np.empty((nsteps, cm.size), np.complex128)
    bnd = np.empty(nsteps)
    c = np.arange(M)
    levels = int(np.ceil(np.log2(M)))
    with np.errstate(invalid="ignore"):
        for i0 in range(0, nsteps, _BLOCK):
            n = min(_BLOCK, nsteps - i0)
            z, a = _branches(h, x, M, R, i0, n)
            u = np.fft.ifft(z, axis=1) * M
            if R != M:
                i = (i0 + np.arange(n, dtype=np.int64))[:, None]
                u = u * np.exp(2j * np.pi * ((c[None, :] * i * (M - R)) % M) / M)
            out[i0:i0 + n] = u[:, cm]
            bnd[i0:i0 + n] = K_SIGMA * U * np.sqrt((a * a).sum(axis=1)) * np.sqrt(9.0 * levels + P + 2.0)
    return out.reshape(-1), bnd


def channelize_literal(h, M, R, ch_map, x_hist, nsteps):
    """the second form: the double sum over k as it stands (small cases)"""
    h = np.asarray(h, np.float32).astype(np.float64)
    x = np.asarray(x_hist).astype(np.complex64).astype(np.complex128)
    K = h.size
    kk = np.arange(K)
    out = np.zeros((nsteps, len(ch_map)), np.complex128)
    for i in range(nsteps):
        seg = x[i * R + K - 1 - kk] * h
        for q, c in enumerate(ch_map):
            out[i, q] = np.sum(seg * np.exp(2j * np.pi * c * (kk + i * (M - R)) / M))
    return out.reshape(-1)


def errors(got, want):
    got = np.asarray(got).astype(np.complex128)
    return np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))


def worst(got, want, bnd, nmap):
    """largest error / bound over all components (a NaN gives inf)"""
    err = errors(got, want).reshape(-1, nmap)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd[:, None])
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def within(got, want, bnd, nmap):
    return bool(np.all(errors(got, want).reshape(-1, nmap) <= bnd[:, None]))


def old_metric(got, want):
    return float(np.abs(np.asarray(got).astype(np.complex128) - want).max() / np.abs(want).max())


def with_rounded_twiddles(h, M, R, ch_map, x_hist, nsteps, bits=16):
    """the planted error: float64 branch sums, the M-point DFT as a direct sum whose twiddles are rounded to `bits` significand bits"""
    from fir_ref import round_mantissa
    h = np.asarray(h, np.float32).astype(np.float64)
    x = np.asarray(x_hist).astype(np.complex64).astype(np.complex128)
    z, _ = _branches(h, x, M, R, 0, nsteps)
    j, c = np.arange(M)[:, None], np.asarray(ch_map, np.int64)[None, :]
    out = np.empty((nsteps, c.size), np.complex128)
    for i in range(nsteps):
        ang = 2.0 * np.pi * ((c * (j + i * (M - R))) % M) / M
        w = round_mantissa(np.cos(ang), bits) + 1j * round_mantissa(np.sin(ang), bits)
        out[i] = z[i] @ w
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- which steps an item reaches

def reach(K, M, R, nsteps, items, rows=None):
    """bool[nsteps]: the steps i with i R <= s < i R + K for some s of `items`; rows = PR: with the window stretched to PR M items towards
    the past (the taps per arm rounded up to PR with zeros), i.e. i R + K - PR M <= s < i R + K"""
    i = np.arange(nsteps, dtype=np.int64) * R
    lo = i if rows is None else i + K - rows * M
    hit = np.zeros(nsteps, bool)
    for s in items:
        hit |= (lo <= s) & (s < i + K)
    return hit


def plant_positions(K, M, R, nsteps, tile_steps):
    """the first item of the buffer, the last item of the history (the K - R items in front of the first new one), an item just in front of
    the route's second tile or range (its reach straddles the boundary), the last item the call reads; (positions, index of the +Inf)"""
    last = (nsteps - 1) * R + K - 1
    pos = [0]
    if K - R - 1 > 0:
        pos.append(K - R - 1)
    P = -(-K // M)
    mid = (tile_steps - max(1, P // 2)) * R + K - 1 - M // 2   # (the steps it reaches begin max(1, P / 2) steps in front of the boundary)
    if pos[-1] < mid < last:
        pos.append(mid)
    pos.append(last)
    return pos, (pos.index(mid) if mid in pos else 0)


def plant(x_hist, positions, inf_at):
    x = np.array(x_hist, np.complex64)
    for i, s in enumerate(positions):
        x[s] = complex(np.inf, np.inf) if i == inf_at else complex(np.nan, np.nan)
    return x
