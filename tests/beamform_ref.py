"""The yardstick of clBeamformer: the contract of include/mi355_clenabled.h in numpy integer arithmetic (numpy.einsum on int64 real and
imaginary planes).  Voltage beams are exact integers, then cast to complex64; power is an int64 sum, then astype(float32) (round to
nearest even).  The bounds that make both exact -- every component below 2^24, every power sum below 2^63 -- are asserted for the
inputs given, so a case outside them fails here and not in a comparison.

Layouts: frames x[t][s][f][p]{I, Q} int8, weights w[f][p][b][s]{re, im} int8 in -127 .. 127, voltage y[t][b][f][p], power P[W][b][f][p]
(P[W][b][f] with stokes_i)."""
import numpy as np

VOLTAGE, POWER = 0, 1


def frames(rng, T, S, F, npol):
    """seeded full-range int8 frames, -128 included"""
    return rng.integers(-128, 128, size=(T, S, F, npol, 2), dtype=np.int8)


def weights(rng, S, F, npol, B):
    return rng.integers(-127, 128, size=(F, npol, B, S, 2), dtype=np.int8)


def extremes(T, S, F, npol, B):
    """x = -128 throughout; w = +-127 in the sign pattern that maximises |re|: re = w_re I - w_im Q with I = Q = -128 is largest in
    magnitude for w_re = -127, w_im = +127: S 2 127 128"""
    x = np.full((T, S, F, npol, 2), -128, np.int8)
    w = np.empty((F, npol, B, S, 2), np.int8)
    w[..., 0] = -127
    w[..., 1] = 127
    return x, w


def voltage_int(x, w):
    """(re, im) int64 planes [t][b][f][p]"""
    assert x.dtype == np.int8 and w.dtype == np.int8 and x.shape[-1] == 2 and w.shape[-1] == 2
    assert w.min() >= -127, "a weight of -128 is outside the contract"
    xi, xq = x[..., 0].astype(np.int64), x[..., 1].astype(np.int64)
    wr, wi = w[..., 0].astype(np.int64), w[..., 1].astype(np.int64)
    re = np.einsum("fpbs,tsfp->tbfp", wr, xi) - np.einsum("fpbs,tsfp->tbfp", wi, xq)
    im = np.einsum("fpbs,tsfp->tbfp", wr, xq) + np.einsum("fpbs,tsfp->tbfp", wi, xi)
    assert max(np.abs(re).max(initial=0), np.abs(im).max(initial=0)) < 1 << 24, "a component reaches 2^24"
    return re, im


def voltage(x, w):
    """complex64 [t][b][f][p], every value an exact integer"""
    re, im = voltage_int(x, w)
    y = np.empty(re.shape, np.complex64)
    y.real = re.astype(np.float32)
    y.imag = im.astype(np.float32)
    assert np.array_equal(y.real.astype(np.int64), re) and np.array_equal(y.imag.astype(np.int64), im)
    return y


def power_int(x, w, Ti, stokes_i=False):
    """int64 sums [W][b][f][p] ([W][b][f] with stokes_i) over windows of Ti frames; x holds a whole number of windows"""
    re, im = voltage_int(x, w)
    T = re.shape[0]
    assert T % Ti == 0 and 1 <= Ti <= 4096
    # int64 would wrap silently: bound the sum in Python integers first
    per_frame = int(np.abs(re).max(initial=0)) ** 2 + int(np.abs(im).max(initial=0)) ** 2
    assert per_frame * Ti * (2 if stokes_i else 1) < 1 << 63, "a power sum reaches 2^63"
    p = (re * re + im * im).reshape((T // Ti, Ti) + re.shape[1:]).sum(axis=1)
    if stokes_i:
        assert p.shape[-1] == 2, "stokes_i needs npol = 2"
        p = p.sum(axis=-1)
    return p


def power(x, w, Ti, stokes_i=False):
    return power_int(x, w, Ti, stokes_i).astype(np.float32)


def plan(mode, npol, S, F, B, Ti=1, stokes_i=False):
    """(frame_bytes, frames_per_unit, out_bytes_per_unit)"""
    if mode == VOLTAGE:
        return 2 * S * F * npol, 1, 8 * B * F * npol
    return 2 * S * F * npol, Ti, 4 * B * F * (1 if stokes_i else npol)
