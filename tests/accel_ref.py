"""Yardstick of clAccelResampler (include/mi355_clenabled.h): the index map with Python integers, the gather with numpy on uint32.

    d(i) = i (N - i);  delta(i) = floor((c d(i) + 2^63) / 2^64);  src(i) = i + delta(i);  out[s][a][i] = in[s][src_a(i)]

Python's // on integers is the floor division the contract names.  Nothing here is floating point but accel_exact's Fractions and the
simulated signals of the chain test."""
from fractions import Fraction

import numpy as np

LIGHT = 299792458
TILE = 1024          # outputs per tile of the tiled route
LDS_WORDS = 4096     # its LDS budget; a window holds at most ONE_TRIAL + ceil((cmax - cmin) N^2 / 2^66) words
ONE_TRIAL = 1544
MAX_GROUP = 16


def cmax(N):
    """the largest legal coefficient: |c| N <= 2^63"""
    return (1 << 63) // N


def delta(N, c, i):
    return (c * i * (N - i) + (1 << 63)) >> 64


def src(N, c, i0=0, count=None):
    """src(i) for i0 <= i < i0 + count as a list of Python integers"""
    count = N - i0 if count is None else count
    return [i + ((c * i * (N - i) + (1 << 63)) >> 64) for i in range(i0, i0 + count)]


def src_array(N, c):
    """the same for a whole series as int64, vectorised and still exact: |c| d + K in 32-bit limbs held in uint64, where
    floor((c d + 2^63) / 2^64) = (|c| d + 2^63) >> 64 for c >= 0 and -((|c| d + 2^63 - 1) >> 64) for c < 0.  tests/test_accel.py compares
    it with src() on whole rows and, at N = 2^22, on windows"""
    u, M = np.uint64, np.uint64(0xFFFFFFFF)
    i = np.arange(N, dtype=np.uint64)
    d = i * (u(N) - i)
    m, K = abs(int(c)), (1 << 63) - (1 if c < 0 else 0)
    m0, m1, d0, d1 = u(m & 0xFFFFFFFF), u(m >> 32), d & M, d >> u(32)
    p00, p01, p10, p11 = m0 * d0, m0 * d1, m1 * d0, m1 * d1          # each below 2^64
    t0 = (p00 & M) + u(K & 0xFFFFFFFF)
    t1 = (p00 >> u(32)) + (p01 & M) + (p10 & M) + u(K >> 32) + (t0 >> u(32))
    t2 = (p01 >> u(32)) + (p10 >> u(32)) + (p11 & M) + (t1 >> u(32))
    q = ((t2 & M) + (((p11 >> u(32)) + (t2 >> u(32))) << u(32))).astype(np.int64)   # (|c| d + K) >> 64, below 2^41
    return i.astype(np.int64) + (-q if c < 0 else q)


def src_truncating(N, c):
    """another function: the quotient truncated toward zero instead of the floor"""
    out = []
    for i in range(N):
        p = c * i * (N - i) + (1 << 63)
        out.append(i + (p // (1 << 64) if p >= 0 else -((-p) // (1 << 64))))
    return out


def resample(x, trials, a0=0, na=None):
    """x[S][N] of any 4-byte dtype -> uint32 [S][na][N], words moved"""
    x = np.ascontiguousarray(x)
    S, N = x.shape
    na = len(trials) - a0 if na is None else na
    w = x.view(np.uint32)
    out = np.empty((S, na, N), np.uint32)
    for t in range(na):
        out[:, t, :] = w[:, src_array(N, int(trials[a0 + t]))]
    return out


def pitched(x, pitch, fill=0x7FC00000):
    """rows of x (uint32 [R][N]) at `pitch` words, NaN words in the gaps, without a gap behind the last row"""
    R, N = x.shape
    buf = np.full((R - 1) * pitch + N, fill, np.uint32)
    for r in range(R):
        buf[r * pitch:r * pitch + N] = x[r]
    return buf


def unpitched(buf, R, N, pitch):
    return np.stack([buf[r * pitch:r * pitch + N] for r in range(R)])


def apex(N, m=1):
    """the smallest c with c dmax / 2^64 >= m + 1/2, dmax = floor(N/2) ceil(N/2) the largest d (for an even N: (N/2)^2): only the
    samples next to N / 2 take the shift m + 1, all others at most m"""
    dmax = (N // 2) * (N - N // 2)
    return -((-((2 * m + 1) << 63)) // dmax)


def apex_run(N, c, m=1):
    """(first, last) sample whose shift is m + 1 under apex(N, m)"""
    at = [i for i in range(N // 2 - 64, N // 2 + 65) if delta(N, c, i) == m + 1]
    assert at and at == list(range(at[0], at[-1] + 1)) and delta(N, c, at[0] - 1) == m and delta(N, c, at[-1] + 1) == m
    return at[0], at[-1]


def lane_runs(N, out_word):
    """the tiled route's partition of a row whose first output lies at word address `out_word`: the outputs in front of the row's first
    16-byte boundary of `out` one by one, then runs of four from boundary to boundary (a trial's tiles meet on boundaries), then the
    rest one by one: [(first, last)]"""
    oh = (4 - out_word % 4) % 4
    nq = (N - oh) // 4
    return ([(k, k) for k in range(oh)] + [(oh + 4 * q, oh + 4 * q + 3) for q in range(nq)] + [(k, k) for k in range(oh + 4 * nq, N)])


def group(N, trials):
    """the tiled route's group size: the largest g <= 16 at which every run of g consecutive trials fits the LDS budget"""
    best = 1
    for g in range(2, min(MAX_GROUP, len(trials)) + 1):
        for a in range(len(trials) - g + 1):
            lo, hi = min(trials[a:a + g]), max(trials[a:a + g])
            if ONE_TRIAL + -((-(hi - lo) * N * N) >> 66) > LDS_WORDS:
                return best
        best = g
    return best


def window_words(N, trials, i0):
    """words of the source window of a group of trials at the tile that starts at i0 (it serves outputs i0 - 3 .. i0 + TILE - 1)"""
    ilo, i1 = max(i0 - 3, 0), min(i0 + TILE, N) - 1
    return i1 + delta(N, max(trials), i1) - (ilo + delta(N, min(trials), ilo)) + 1


def coeff_exact(tsamp_s, accel_m_s2):
    """-2^64 accel tsamp / (2 c_light) as the exact rational of the double inputs"""
    return -Fraction(accel_m_s2) * Fraction(tsamp_s) * (1 << 64) / (2 * LIGHT)


def words(rng, S, N):
    """random uint32 words, unique per (series, sample) as far as 32 bits allow, with NaN patterns, +-Inf, -0 and subnormals among them"""
    w = rng.permutation(np.arange(1 << 22, (1 << 22) + S * N, dtype=np.uint64) * np.uint64(1021) % np.uint64(1 << 32)).astype(np.uint32)
    w = w.reshape(S, N)
    special = [0x7FC00002, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00000000]
    for k, v in enumerate(special):
        w[k % S, (k * 37 + 5) % N] = v
        w[(k + 1) % S, N - 1 - (k * 29) % (N // 2)] = v
    return w


def pulse_train(N, period, c_distort):
    """a train of one-sample pulses every `period` samples, seen through the map of c_distort: y[i] = train[src(i)]"""
    t = np.arange(N)
    train = (((t + 0.5) % period) < 1.0).astype(np.float32)
    return train[src_array(N, c_distort)]
