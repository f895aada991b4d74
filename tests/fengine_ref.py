"""The yardstick of clFEngine: the contract of include/mi355_clenabled.h restated in float64 numpy, plus what a test needs to compare a
float32 device with it honestly -- per output component the distance d from the float64 value to the nearest decision boundary of the
quantiser (the half-integers up to +-127.5; beyond +-127.5 nothing but +-127.5 itself) and a bound delta on the float32 error.

    z[n] = sum_{p<P} h[p F + n] x_r[(t + p) F + n]         X[f] = sum_n z[n] exp(-2 pi j f n / F)         v = gain[r][f] X[f]
    out[t][s][f'][p] = {sat(rint(v.re)), sat(rint(v.im))}   r = s npol + p,  f' = shift ? (f + F/2) mod F : f,  rint = half to even

delta (see `Result.delta`): with u = 2^-24 every float32 operation errs by at most u times its result.  The P products and adds of
an arm sum err by at most sqrt(P) u a[n] in the root-sum-square sense, a[n] = sum_p |h[p F + n]| |x[(t + p) F + n]| >= |z[n]|.  A
transform of F points is ceil(log2 F) radix-2 levels (a higher radix only merges levels); on the way to one output a value passes
one twiddle product (two products and an add against a table value rounded to float32: at most 2.4 u) and one add (u) per level, less
than 3 u together.  The errors of different operations are taken as independent and zero-mean, so their squares add, and the squares
of the partial sums of a level add up to no more than Q^2 = sum_n a[n]^2 (each partial sum is a sum of z's whose cross terms have zero
mean for the random inputs this bound is used with).  With the gain product and one spare operation that gives

    sigma <= u |gain| Q sqrt(9 ceil(log2 F) + P + 2),          delta = 8 sigma.

sigma over-states the standard deviation (it uses each operation's largest error, not its rms u / sqrt(3), and a[n] for |z[n]|), and
eight of them leave a probability below 1e-15 per component.  Everything in delta comes from the inputs, the taps and the gains.
"""
import numpy as np

U = 2.0 ** -24
K_SIGMA = 8.0


class Result:
    """out: int8 [T][S][F][npol][2]; v: complex128 [T][S][F][npol] (the value before rounding, channel order of the output);
    d, delta: float64 like out; clip: bool like out; clips(mask): per-input counts"""

    def __init__(self, out, v, d, delta, clip, npol):
        self.out, self.v, self.d, self.delta, self.clip, self.npol = out, v, d, delta, clip, npol

    def decided(self):
        """components whose float64 value is further from every boundary than the float32 error bound"""
        return self.d > self.delta

    def clips(self, mask=None):
        """clip count per input r = s npol + p, over the components in `mask` (all by default)"""
        c = self.clip if mask is None else (self.clip & mask)
        T, S, F, npol, _ = c.shape
        return c.sum(axis=(0, 2, 4)).reshape(S * npol).astype(np.uint64)

    def undecided_per_input(self):
        u = ~self.decided()
        T, S, F, npol, _ = u.shape
        return u.sum(axis=(0, 2, 4)).reshape(S * npol)


def distance(v):
    """distance of real float64 values to the nearest decision boundary; inf for NaN (a NaN is 0 and a clip, whatever the arithmetic)"""
    a = np.abs(v)
    with np.errstate(invalid="ignore"):  # inf - inf on the branch an infinite value does not take
        inside = np.abs((a - np.floor(a)) - 0.5)
        d = np.where(a > 127.5, a - 127.5, np.minimum(inside, 127.5 - a))
    return np.where(np.isnan(v), np.inf, d)


def quantise(v):
    """(int8 value, clipped) of real float64 values"""
    r = np.rint(v)
    nan = np.isnan(v)
    clip = nan | (np.abs(r) > 127)
    q = np.where(nan, 0, np.clip(r, -127, 127)).astype(np.int8)
    return q, clip


def spectra(xs, h, F, P, T):
    """X [R][T][F] complex128 and Q [R][T] of R history-prefixed streams (each (T + P - 1) F items)"""
    xs = [np.asarray(x, np.complex128) for x in xs]
    h = np.asarray(h, np.float64).reshape(P, F)
    R = len(xs)
    X = np.empty((R, T, F), np.complex128)
    Q = np.empty((R, T), np.float64)
    for r, x in enumerate(xs):
        assert x.size >= (T + P - 1) * F
        fr = x[:(T + P - 1) * F].reshape(T + P - 1, F)
        z = np.zeros((T, F), np.complex128)
        a = np.zeros((T, F), np.float64)
        for p in range(P):
            z += h[p] * fr[p:p + T]
            a += np.abs(h[p]) * np.abs(np.nan_to_num(fr[p:p + T], nan=0.0))
        X[r] = np.fft.fft(z, axis=1)
        Q[r] = np.sqrt((a * a).sum(axis=1))
    return X, Q


def fengine(xs, h, gains, S, npol, F, P, shift, T):
    """the frames of T calls' worth of input: a Result"""
    R = S * npol
    assert len(xs) == R and (not shift or F % 2 == 0)
    g = np.ones((R, F)) if gains is None else np.asarray(gains, np.float64).reshape(R, F)
    h = np.ones(P * F) if h is None else h
    X, Q = spectra(xs, h, F, P, T)
    v = g[:, None, :] * X                                   # [R][T][F]
    levels = int(np.ceil(np.log2(F)))
    dl = K_SIGMA * U * np.abs(g)[:, None, :] * Q[:, :, None] * np.sqrt(9.0 * levels + P + 2.0)
    if shift:
        idx = (np.arange(F) + F // 2) % F
        v, dl = v[:, :, idx], dl[:, :, idx]                 # position f' holds channel (f' + F/2) mod F
    # [R][T][F] -> [T][S][F][npol]
    v = v.reshape(S, npol, T, F).transpose(2, 0, 3, 1)
    dl = dl.reshape(S, npol, T, F).transpose(2, 0, 3, 1)
    comp = np.stack([v.real, v.imag], axis=-1)
    out, clip = quantise(comp)
    delta = np.stack([dl, dl], axis=-1)
    return Result(out, v, distance(comp), delta, clip, npol)


def sinc_taps(F, P):
    """a Hamming-windowed sinc prototype of P F taps, one channel wide (the usual radio-astronomy bank); P = 1: the Hamming window"""
    n = np.arange(P * F)
    t = (n - (P * F - 1) / 2.0) / F
    return (np.sinc(t) * np.hamming(P * F)).astype(np.float32)
