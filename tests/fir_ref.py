"""The yardstick of clFilter / clComplexFilter in direct form: plain numpy, float64.  Plain module (no fixtures), shared by
tests/test_fir_ref.py (CPU), tests/test_filter_window_gpu.py and the filter cases of tests/switch_cases.py.

Contract (include/mi355_clenabled.h): taps h[0..K), decimation D, `x_hist` the history-prefixed input (x_hist[K-1] is x[0]).  Output m
reads the items [m D, m D + K) of it:

    y[m] = sum_k h[k] x_hist[m D + K-1-k]

Taps and inputs are rounded to float32 BEFORE the float64 evaluation, so quantisation is not part of any error measured here.

The tolerance (`bound`), per output and per component.  A component is a sum of n float32 terms t_k: n = K terms h[k] x.re for real taps,
n = 2 K terms (h.re x.re, -h.im x.im) for complex ones.  With u = 2^-24 every float32 addition errs by at most u times its partial sum,
rms u / sqrt(3) of it; the partial sum after i of n terms has the mean square (i / n) T^2, T^2 = sum_k t_k^2, for terms of random sign;
the additions' errors are taken as independent, so their squares add:

    sigma^2 = sum_i (u^2 / 3) (i / n) T^2 = u^2 (n / 6) T^2,        sigma = u sqrt(n / 6) T.

The products' own roundings (absent with fused multiply-adds) add u^2 T^2 / 3 at most and are left to the multiple.  Plain forward float32
summation WITHOUT fused multiply-adds -- the worst order a kernel may use -- reaches 6.6 sigma at most over the shapes measured (K = 9 ...
9000, DESIGN.md "Tolerances"; tests/test_fir_ref.py prints the ratios of this grid), so

    bound = MULT sigma + u |y|,        MULT = 16

leaves every CPU order under half of it; u |y| is the rounding of the result itself.  Everything in it comes from taps and samples.
"""
import numpy as np

U = 2.0 ** -24
MULT = 16.0
PAD = 18  # items a non-finite sample may reach beyond the windows that hold it (include/mi355_clenabled.h; the largest over the kernels)

# (K, D, complex taps) of every value test, by the kernel that takes the shape (tests/test_filter_window_gpu.py says how each is reached)
_EVEN = ((65, 4, False), (65, 16, False), (200, 32, True))
_ODD = ((65, 9, False), (77, 15, True), (33, 33, False))
GRID = {
    "k_fir_td": ((1, 1, False), (9, 1, False), (15, 1, True), (9, 3, False), (65, 2, False)),
    "k_fir_mfma_all": ((16, 1, False), (65, 1, False), (129, 1, False), (65, 1, True)),
    "k_fir_mfma_dec": ((129, 2, False), (200, 8, True), (200, 3, True)),
    "k_fir_dec2_even": _EVEN,
    "k_fir_dec2_odd": _ODD,
    "k_fir_dec_lds": ((65, 10, False),) + _EVEN[1:] + _ODD + ((65, 3001, False),),
    "k_fir_td_dec": ((33, 600, False), (65, 40, False)),
}


def tile_items(kernel, K, D):
    """input items per tile of a kernel, from the constants of csrc/filter.hip: k_fir_td kTdTile = 256 x 8 = 2048 undecimated outputs,
    k_fir_mfma kMfTile = 4096, k_fir_dec2 tile_out outputs (a span of 3072 samples up to 128 taps, 4096 above, less the taps rounded up to 8,
    over D, plus one; whole rounds of kD2Threads = 256 above that; even for an odd D), k_fir_dec_lds (kDlSpan = 8192 - K) / D + 1 outputs (2048
    at most), k_fir_td_dec 256 outputs per workgroup"""
    if kernel == "k_fir_td":
        return 2048
    if kernel.startswith("k_fir_mfma"):
        return 4096
    if kernel.startswith("k_fir_dec2"):
        KP = (K + 7) // 8 * 8
        t = min(((3072 if K <= 128 else 4096) - KP) // D + 1, 2048)
        if t > 256:
            t = t // 256 * 256
        if D % 2 and t > 1:
            t &= ~1
        return t * D
    if kernel == "k_fir_dec_lds":
        return min((8192 - K) // D + 1, 2048) * D
    assert kernel == "k_fir_td_dec"
    return 256 * D


def nout(kernel, K, D):
    """outputs of a value test: two tiles of the kernel and a ragged third"""
    return 2 * max(tile_items(kernel, K, D) // D, 1) + 37


def cases():
    """every (kernel, K, D, complex) of the grid"""
    return [(kern,) + s for kern, v in GRID.items() for s in v]


def crandn(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


def make_taps(K, complex_taps=False, seed=0):
    """seeded standard normal, NOT a designed low-pass (a wrong tap, order or offset shows at full scale: resampler_ref.make_taps), and no
    exact zero (a zero tap would hide a read of the wrong sample)"""
    rng = np.random.default_rng(4000 + 7 * K + seed)
    h = crandn(rng, K) if complex_taps else rng.standard_normal(K).astype(np.float32)
    assert np.all(h.real != 0) and (not complex_taps or np.all(h.imag != 0))
    return h


def make_input(K, D, n, seed=0):
    """exactly the n D + K - 1 items a call reads, history (non-zero) included"""
    return crandn(np.random.default_rng(91 + seed), n * D + K - 1)


def _f64(a):
    a = np.asarray(a)
    return a.astype(np.complex64).astype(np.complex128) if np.iscomplexobj(a) else a.astype(np.float32).astype(np.float64)


_BLOCK = 1 << 14


def windows(K, D, n, m0=0):
    """idx[n][K]: idx[m][i] = (m0 + m) D + i, the items output m0 + m reads, ascending (tap K-1-i multiplies item i of the window)"""
    return ((m0 + np.arange(n, dtype=np.int64)) * D)[:, None] + np.arange(K, dtype=np.int64)[None, :]


def fir(h, x_hist, D, n):
    """y complex128: the formula above, literally"""
    h = _f64(h)
    K = h.size
    x = _f64(x_hist).astype(np.complex128)
    assert x.size >= (n - 1) * D + K
    hr = h[::-1]
    y = np.empty(n, np.complex128)
    for m0 in range(0, n, _BLOCK):
        k = min(_BLOCK, n - m0)
        y[m0:m0 + k] = x[windows(K, D, k, m0)] @ hr
    return y


def fir_by_convolve(h, x_hist, D, n):
    """the second, independent form: np.convolve over the whole buffer, then every D-th value"""
    h = _f64(h)
    x = _f64(x_hist).astype(np.complex128)
    full = np.convolve(x, h.astype(np.complex128))
    return full[h.size - 1 + np.arange(n, dtype=np.int64) * D]


def _terms(h, x_hist, D, n, dtype):
    """(re[n][nt], im[n][nt]): the terms of both components in the order of the taps k = K-1 ... 0 (the items of the window ascending)"""
    h = np.asarray(h)
    K = h.size
    W = np.asarray(x_hist)[windows(K, D, n)]
    hr = h[::-1]
    f = dtype
    wr, wi = W.real.astype(f), W.imag.astype(f)
    if np.iscomplexobj(h):
        ar, ai = hr.real.astype(f)[None, :], hr.imag.astype(f)[None, :]
        re = np.stack([ar * wr, -(ai * wi)], axis=2).reshape(n, -1)
        im = np.stack([ar * wi, ai * wr], axis=2).reshape(n, -1)
    else:
        a = hr.astype(f)[None, :]
        re, im = a * wr, a * wi
    return re, im


def bound(h, x_hist, D, n):
    """[n][2] float64: the tolerance of (re, im) of every output, from taps and samples alone (the model in the module docstring)"""
    out = np.empty((n, 2))
    y = fir(h, x_hist, D, n)
    for m0 in range(0, n, _BLOCK):
        k = min(_BLOCK, n - m0)
        xs = _f64(x_hist)[m0 * D:]
        re, im = _terms(_f64(h), xs, D, k, np.float64)
        nt = re.shape[1]
        out[m0:m0 + k, 0] = MULT * U * np.sqrt(nt / 6.0) * np.sqrt((re * re).sum(axis=1))
        out[m0:m0 + k, 1] = MULT * U * np.sqrt(nt / 6.0) * np.sqrt((im * im).sum(axis=1))
    out[:, 0] += U * np.abs(y.real)
    out[:, 1] += U * np.abs(y.imag)
    return out


def errors(got, want):
    """[n][2]: |got - want| per component (NaN where got is not finite)"""
    got = np.asarray(got).astype(np.complex128)
    return np.stack([np.abs(got.real - want.real), np.abs(got.imag - want.imag)], axis=1)


def within(got, want, bnd):
    """every component of every output within its bound (NaN fails)"""
    return bool(np.all(errors(got, want) <= bnd))


def worst(got, want, bnd):
    """largest error / bound over all components (0 / 0 counts as 0; a NaN gives inf)"""
    err = errors(got, want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def old_metric(got, want):
    """the whole-call metric the older tests use (conftest.relerr): max |got - want| / max |want|"""
    return float(np.abs(np.asarray(got).astype(np.complex128) - want).max() / np.abs(want).max())


def float32_orders(h, x_hist, D, n):
    """the formula in float32 arithmetic without fused multiply-adds, terms summed forward, reversed and pairwise: {name: y complex128}"""
    f = np.float32
    re, im = _terms(np.asarray(h), np.asarray(x_hist).astype(np.complex64), D, n, f)

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


def truncate_mantissa(a, bits=16):
    """float32 (or complex64) values with the significand cut to `bits` bits (the low 24 - bits bits zeroed): a kernel whose operands lost
    eight mantissa bits"""
    a = np.ascontiguousarray(a)
    v = a.view(np.float32).copy()
    v.view(np.uint32)[...] &= np.uint32((0xFFFFFFFF << (24 - bits)) & 0xFFFFFFFF)
    return v.view(a.dtype)


def round_mantissa(a, bits=16):
    """float64 values rounded to the nearest value with a significand of `bits` bits"""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    return np.ldexp(np.rint(m * 2.0 ** bits) / 2.0 ** bits, e)


# ---------------------------------------------------------------------------------------------------------------- which outputs an item reaches

def reach(K, D, n, items, pad=0):
    """bool[n]: the outputs m with m D - pad <= s < m D + K + pad for some s of `items` (pad = 0: the outputs whose window holds one)"""
    m = np.arange(n, dtype=np.int64) * D
    hit = np.zeros(n, bool)
    for s in items:
        hit |= (m - pad <= s) & (s < m + K + pad)
    return hit


def plant_positions(K, D, n, tile_items):
    """where the reach test plants its non-finite items: the first item of the buffer, the last item of the history, an item whose reach
    straddles the boundary between the route's first two tiles (tile_items input items per tile), the last item the outputs read.  Returns
    (positions, index of the one that is +Inf).  Apart from the first two (K - 2 items apart by their definition) they are further apart than
    K + 2 PAD wherever the call is long enough."""
    last = (n - 1) * D + K - 1
    pos = [0]
    if K >= 2 and K - 2 not in pos:
        pos.append(K - 2)
    mid = min(max(tile_items + K // 2, K + 2 * PAD + K), last)
    if all(abs(mid - p) > K + 2 * PAD for p in pos) and last - mid > K + 2 * PAD:
        pos.append(mid)
    if last not in pos:
        pos.append(last)
    inf_at = pos.index(mid) if mid in pos else len(pos) - 1
    return pos, inf_at


def plant(x_hist, positions, inf_at):
    x = np.array(x_hist, np.complex64)
    for i, s in enumerate(positions):
        x[s] = complex(np.inf, np.inf) if i == inf_at else complex(np.nan, np.nan)
    return x
