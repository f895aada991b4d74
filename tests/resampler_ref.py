"""The yardstick of clRationalResampler: plain numpy, float64, vectorised per arm.  Plain module (no fixtures), shared by
tests/test_resampler.py (CPU) and tests/test_resampler_gpu.py.

Contract (include/mi355_clenabled.h): taps h[0..K), interpolation L, decimation M, nt = ceil(K / L), hp = h zero-padded to
nt L, arm p = hp[p + L j].  Input history-prefixed: in[nt-1] is x[0].  Output m of a call that starts at phase c:

    q = c + m M;  p = q mod L;  b = q div L;     y[m] = sum_j hp[p + L j] in[nt-1 + b - j]

Taps and inputs are rounded to float32 BEFORE the float64 evaluation, so quantisation is not part of any error measured here.
"""
import numpy as np

RATES = ((1, 1), (2, 1), (3, 1), (8, 1), (1, 3), (3, 2), (2, 3), (7, 5), (5, 7), (16, 1), (64, 3), (160, 147), (147, 160))
LONG = ((3, 2, 391), (160, 147, 3840))   # nt = 131 crosses any unroll-by-8 and any arm-tile edge; the 160/147 design length
NOUT = (1, 2, 63, 64, 65, 255, 256, 257, 20011)
COMPLEX_RATES = ((2, 1), (3, 2), (7, 5), (160, 147))
U = 2.0 ** -24


def ks(L):
    """tap counts per rate: arms that are all padding, K no multiple of L, nt = 1"""
    out = []
    for k in (1, L - 1, L, L + 1, 4 * L + 3, 89):
        if k >= 1 and k not in out:
            out.append(k)
    return out


def phases(L):
    return sorted({0, L // 2, L - 1})


def grid():
    """every (L, M, K) of the value tests"""
    return [(L, M, K) for L, M in RATES for K in ks(L)] + list(LONG)


def case_id(c):
    return "-".join(str(v) for v in c)


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def make_taps(K, complex_taps=False, seed=0):
    """seeded standard normal, NOT a designed low-pass: a wrong arm, order or offset shows at full scale"""
    rng = np.random.default_rng(1000 + 7 * K + seed)
    if complex_taps:
        return crandn(rng, K)
    return rng.standard_normal(K).astype(np.float32)


def rrc(gain, sps, alpha, ntaps):
    """root-raised-cosine taps (the textbook closed form, as gr::filter::firdes::root_raised_cosine evaluates it), unit-sum scaled
    by `gain`"""
    t = (np.arange(ntaps) - ntaps // 2) / float(sps)
    out = np.empty(ntaps)
    for i, x in enumerate(t):
        den = 1.0 - (4.0 * alpha * x) ** 2
        if abs(den) < 1e-9:
            out[i] = alpha / np.sqrt(2.0) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * alpha)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * alpha)))
        elif x == 0.0:
            out[i] = 1.0 - alpha + 4.0 * alpha / np.pi
        else:
            out[i] = (np.sin(np.pi * x * (1 - alpha)) + 4 * alpha * x * np.cos(np.pi * x * (1 + alpha))) / (np.pi * x * den)
    return (gain * out / out.sum()).astype(np.float32)


def taps_per_arm(K, L):
    return -(-K // L)


def arms(h, L):
    """[L][nt]: arm p is hp[p + L j]"""
    h = np.asarray(h)
    nt = taps_per_arm(h.size, L)
    hp = np.zeros(nt * L, h.dtype)
    hp[:h.size] = h
    return hp.reshape(nt, L).T.copy()


def plan(L, M, K, c, n):
    """(nt, consumed, needed, phase_after), python integers (unbounded)"""
    nt = taps_per_arm(K, L)
    adv = c + n * M
    return nt, adv // L, (0 if n == 0 else nt + (c + (n - 1) * M) // L), adv % L


def noutput_for(L, M, K, c, navail):
    nt = taps_per_arm(K, L)
    return 0 if navail < nt else ((navail - nt + 1) * L - 1 - c) // M + 1


def make_input(L, M, K, c, n, seed=0):
    """exactly `needed` history-prefixed items"""
    return crandn(np.random.default_rng(77 + seed), plan(L, M, K, c, n)[2])


def _f32(a):
    a = np.asarray(a)
    return a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a) else a.astype(np.float32).astype(np.float64)


_BLOCK = 1 << 15  # outputs per gathered block: the window matrix of a long call stays small


def windows(in_hist, L, M, nt, c, n, m0=0):
    """(p[n], W[n][nt]) of outputs m0 .. m0+n-1 with W[m][j] = in[nt-1 + b - j]"""
    q = c + (m0 + np.arange(n, dtype=np.int64)) * M
    p, b = q % L, q // L
    idx = (nt - 1 + b)[:, None] - np.arange(nt)[None, :]
    return p, np.asarray(in_hist)[idx]


def resample(h, L, M, in_hist, n, c):
    """(y complex128, consumed, phase_after): the formula above, literally"""
    A = arms(_f32(h), L)
    nt = A.shape[1]
    x = _f32(in_hist).astype(np.complex128)
    _, consumed, needed, c2 = plan(L, M, np.asarray(h).size, c, n)
    assert x.size >= needed, (x.size, needed)
    y = np.zeros(n, np.complex128)
    for m0 in range(0, n, _BLOCK):
        k = min(_BLOCK, n - m0)
        p, W = windows(x, L, M, nt, c, k, m0)
        yb = y[m0:m0 + k]
        for arm in np.unique(p):
            sel = p == arm
            yb[sel] = W[sel] @ A[arm]
    return y, consumed, c2


def resample_by_stuffing(h, L, M, in_hist, n, c):
    """the second, independent form: zero-stuff the whole history-prefixed buffer, np.convolve, slice"""
    h = _f32(h)
    x = _f32(in_hist).astype(np.complex128)
    nt = taps_per_arm(h.size, L)
    zs = np.zeros(x.size * L, np.complex128)
    zs[::L] = x
    full = np.convolve(zs, h.astype(np.complex128))
    return full[(nt - 1) * L + c + np.arange(n, dtype=np.int64) * M]


def bound(h, L, in_hist, c, M, n):
    """per-output, per-component tolerance: 2 (n_eff + 2) 2^-24 sum_j |hp[p + L j]| max(|Re in|, |Im in|) over the window; n_eff = nt
    for real taps and 2 nt for complex ones, whose |h| is |Re h| + |Im h|.  The order-independent bound n_eff u sum|a||b| of a float32
    dot product evaluated in any order, with or without FMA, plus the final rounding, times 2 for everything second-order."""
    A = arms(_f32(h), L)
    nt = A.shape[1]
    cplx = np.iscomplexobj(A)
    absA = np.abs(A.real) + np.abs(A.imag) if cplx else np.abs(A)
    x = _f32(in_hist).astype(np.complex128)
    mag = np.maximum(np.abs(x.real), np.abs(x.imag))
    n_eff = 2 * nt if cplx else nt
    out = np.empty(n)
    for m0 in range(0, n, _BLOCK):
        k = min(_BLOCK, n - m0)
        p, W = windows(mag, L, M, nt, c, k, m0)
        out[m0:m0 + k] = np.einsum("mj,mj->m", absA[p], W)
    return 2.0 * (n_eff + 2) * U * out


def within(got, want, bnd):
    """every component of every output within its bound (NaN fails)"""
    got = np.asarray(got).astype(np.complex128)
    return bool(np.all(np.abs(got.real - want.real) <= bnd) and np.all(np.abs(got.imag - want.imag) <= bnd))


def worst(got, want, bnd):
    """largest error / bound over all components (a bound of 0 with an error of 0 counts as 0)"""
    got = np.asarray(got).astype(np.complex128)
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    return float(r.max()) if r.size else 0.0


def float32_orders(h, L, M, in_hist, n, c):
    """the formula in float32 arithmetic, terms summed forward, reversed and pairwise: {name: y complex128}"""
    A = arms(np.asarray(h), L)
    nt = A.shape[1]
    x = np.asarray(in_hist).astype(np.complex64)
    p, W = windows(x, L, M, nt, c, n)
    a = A[p]
    f = np.float32
    if np.iscomplexobj(A):
        ar, ai = a.real.astype(f), a.imag.astype(f)
        wr, wi = W.real.astype(f), W.imag.astype(f)
        re = np.stack([ar * wr, -(ai * wi)], axis=2).reshape(n, -1)
        im = np.stack([ar * wi, ai * wr], axis=2).reshape(n, -1)
    else:
        a = a.astype(f)
        re, im = a * W.real.astype(f), a * W.imag.astype(f)

    def forward(t):
        acc = np.zeros(t.shape[0], f)
        for k in range(t.shape[1]):
            acc = (acc + t[:, k]).astype(f)
        return acc

    def pairwise(t):
        size = 1
        while size < t.shape[1]:
            size *= 2
        t = np.concatenate([t, np.zeros((t.shape[0], size - t.shape[1]), f)], axis=1)
        while t.shape[1] > 1:
            t = (t[:, 0::2] + t[:, 1::2]).astype(f)
        return t[:, 0]

    out = {}
    for name, fn in (("forward", forward), ("reversed", lambda t: forward(t[:, ::-1])), ("pairwise", pairwise)):
        out[name] = fn(re).astype(np.float64) + 1j * fn(im).astype(np.float64)
    return out
