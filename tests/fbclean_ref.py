"""The yardstick of clFilterbankCleaner: the contract of include/mi355_clenabled.h in numpy.

  block_sums   step 1: per (r, f) the float64 sums a1_s / a2_s of the 16 segments in ascending t (an explicit loop: one IEEE addition
               per sample, as the contract pins), then the adjacent-pair tree over the 16
  flag         step 2: m, var, sk, good, m32, is32, one numpy float64 operation per operation of the contract (numpy never contracts,
               and its sqrt and division are IEEE correctly rounded)
  clean        steps 1 - 4 over a call: out, cflags, tflags, stats

Float32 steps use numpy float32 arrays, so every operation is one binary32 rounding.  Every comparison with the device is array_equal
on raw bits.  Layout: x[t][r][f] float32."""
import numpy as np

SEG = 16
LANES = 64


def plan(R, F):
    """(floats_per_sample, cflag_bytes_per_block, tflag_bytes_per_sample)"""
    return R * F, R * F, R


def tree(parts):
    """adjacent-pair binary tree over a list of arrays whose length is a power of two"""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0]


def block_sums(xb):
    """(s1, s2) float64 of one block xb[Tb][...] float32"""
    assert xb.dtype == np.float32 and xb.shape[0] % SEG == 0
    L = xb.shape[0] // SEG
    x = xb.astype(np.float64)
    a1, a2 = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(SEG):
            p, q = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
            for i in range(s * L, (s + 1) * L):
                p = p + x[i]
                q = q + x[i] * x[i]
            a1.append(p)
            a2.append(q)
        return tree(a1), tree(a2)


def sequential_sums(xb):
    """what the contract is NOT: plain sequential float64 sums over the block"""
    x = xb.astype(np.float64)
    p, q = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
    for i in range(x.shape[0]):
        p = p + x[i]
        q = q + x[i] * x[i]
    return p, q


def sk_of(s1, s2, Tb, nd):
    M = np.float64(Tb)
    with np.errstate(all="ignore"):
        c = (M * np.float64(nd) + 1.0) / (M - 1.0)
        return c * ((M * s2) / (s1 * s1) - 1.0)


def sk_estimate(col, nd):
    """sk of one column of Tb float32 samples"""
    col = np.ascontiguousarray(col, np.float32)
    s1, s2 = block_sums(col.reshape(-1, 1))
    return sk_of(s1, s2, col.size, nd)[0]


def flag(s1, s2, Tb, nd, sk_lo, sk_hi, mask):
    """(good bool, m32, is32, pos) per (r, f); mask[f] broadcasts along the last axis"""
    M = np.float64(Tb)
    with np.errstate(all="ignore"):
        m = s1 / M
        var = s2 / M - m * m
        sk = sk_of(s1, s2, Tb, nd)
        pos = var > 0
        good = (np.asarray(mask) == 0) & pos & (sk >= np.float64(sk_lo)) & (sk <= np.float64(sk_hi))
        m32 = m.astype(np.float32)
        is32 = (1.0 / np.sqrt(var)).astype(np.float32)
    return good, m32, is32, pos


def zero_dm_sum(y):
    """zs float64 per (t, r) of y[Tb][R][F] float32 (flagged channels already +0.0): 64 partials in ascending f, then the tree"""
    Tb, R, F = y.shape
    G = -(-F // (4 * LANES))
    yp = np.zeros((Tb, R, G * 4 * LANES), np.float64)  # channels past F add +0.0: the same bits
    yp[:, :, :F] = y
    yp = yp.reshape(Tb, R, G, LANES, 4)
    p = np.zeros((Tb, R, LANES))
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            for k in range(4):
                p = p + yp[:, :, g, :, k]
        return tree([p[:, :, j] for j in range(LANES)])


def clean(x, Tb, nd=1.0, sk_lo=-np.inf, sk_hi=np.inf, td=np.inf, zero_dm=0, mask=None):
    """(out[t][r][f] float32, cflags[b][r][f] uint8, tflags[t][r] uint8, stats[b][r][f][2] float32)"""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3 and x.shape[0] % Tb == 0 and Tb % SEG == 0
    n, R, F = x.shape
    nb = n // Tb
    mask = np.zeros(F, np.uint8) if mask is None else np.asarray(mask)
    td2 = np.float64(td) * np.float64(td)
    out = np.empty_like(x)
    cflags = np.empty((nb, R, F), np.uint8)
    tflags = np.zeros((n, R), np.uint8)
    stats = np.empty((nb, R, F, 2), np.float32)
    zero = np.float32(0.0)
    for b in range(nb):
        xb = x[b * Tb:(b + 1) * Tb]
        s1, s2 = block_sums(xb)
        good, m32, is32, pos = flag(s1, s2, Tb, nd, sk_lo, sk_hi, mask)
        cflags[b] = ~good
        stats[b, :, :, 0] = np.where(pos, m32, zero)
        stats[b, :, :, 1] = np.where(pos, is32, zero)
        with np.errstate(all="ignore"):
            y = np.where(good[None], (xb - m32[None]) * is32[None], zero)
            assert y.dtype == np.float32
            if zero_dm:
                zs = zero_dm_sum(y)
                ng = good.sum(axis=1).astype(np.float64)[None, :]
                tf = zs * zs > td2 * ng
                z32 = (zs / ng).astype(np.float32)
                y = np.where(good[None] & ~tf[:, :, None], y - z32[:, :, None], zero)
                assert y.dtype == np.float32
                tflags[b * Tb:(b + 1) * Tb] = tf
        out[b * Tb:(b + 1) * Tb] = y
    return out, cflags, tflags, stats


def gamma(rng, n, R, F, nd=16.0):
    """seeded power data: the mean of nd exponentials per sample, times a bandpass that varies by channel"""
    band = (1.0 + 0.5 * np.sin(np.arange(F) * 0.37)) * 37.0
    return (rng.gamma(nd, 1.0 / nd, (n, R, F)) * band).astype(np.float32)


def wide_range(rng, n, R, F):
    return np.exp2(rng.uniform(-20, 20, (n, R, F))).astype(np.float32)


def search_scene(seed=7):
    """The end-to-end fixture: a gamma-noise filterbank R = 2, F = 256, Tb = 128, a few blocks plus the dedisperser's look-ahead, with
    a pulse 8 samples wide dispersed as trial d0 of a 16-trial table in row r0, a brighter broadband (zero-DM) spike in the same row,
    and one channel with intermittent bursts; the limits are 1 +- 4 (2 / sqrt(M)) and td = 5."""
    import dedisp_ref
    import psearch_ref
    R, F, D, K, Tb, nd = 2, 256, 16, 5, 128, 16.0
    r0, d0, t0, t_spike, f_bad = 1, 9, 200, 333, 77
    tab, H = dedisp_ref.delays(1500.0, -300.0 / F, F, 1e-3, np.arange(D) * 6.0)
    n = 4 * Tb                                # outputs of the search: 4 blocks of the search's own block length Tb
    n_dd = n + psearch_ref.history(K)         # outputs of the dedisperser
    nb_clean = -(-(n_dd + H) // Tb)           # whole cleaner blocks that cover the dedisperser's input
    rng = np.random.default_rng(seed)
    x = gamma(rng, nb_clean * Tb, R, F, nd).astype(np.float64)
    band = x.mean(axis=0)
    sigma = band / np.sqrt(nd)
    for f in range(F):
        x[t0 + tab[d0, f]:t0 + tab[d0, f] + 8, r0, f] += 1.0 * sigma[r0, f]
    x[t_spike:t_spike + 4, r0, :] += 3.5 * sigma[r0]
    for t in range(40, nb_clean * Tb, 97):
        x[t:t + 6, :, f_bad] *= 12.0
    M = float(Tb)
    w = 4.0 * 2.0 / np.sqrt(M)
    return dict(R=R, F=F, D=D, K=K, Tb=Tb, nd=nd, H=H, tab=tab, x=x.astype(np.float32), n=n, n_dd=n_dd, n_clean=nb_clean * Tb, r0=r0, d0=d0, t0=t0,
                t_spike=t_spike, f_bad=f_bad, sk_lo=1.0 - w, sk_hi=1.0 + w, td=5.0,
                inv_sigma=np.full(R * D, 1.0 / np.sqrt(F), np.float32))


def search(sc, x):
    """the reference chain dedisp_ref -> psearch_ref on a filterbank x of the scene: the peak records [block][series]"""
    import dedisp_ref
    import psearch_ref
    y = dedisp_ref.dedisperse(np.ascontiguousarray(x[:sc["n_dd"] + sc["H"]]), sc["tab"], sc["n_dd"], dedisp_ref.TRIAL_MAJOR)
    return psearch_ref.peaks(y.reshape(sc["R"] * sc["D"], sc["n_dd"]), sc["K"], sc["Tb"], sc["n"], None, sc["inv_sigma"])
