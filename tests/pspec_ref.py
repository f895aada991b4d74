"""Numpy float64 yardstick for clPowerSpectrum (the contract: include/mi355_clenabled.h).

  pspec(x, N, K, H, S, window, shift, log_output, scale)   P_s[b] = scale / K * sum_{k < K} |DFT_N(w .* x[(s K + k) H + (0 .. N))][b]|^2,
                                                           float64 throughout, the result rounded to float32, shape (S, N)
  pspec64(...)                                             the same before the rounding (and before the logarithm): the linear spectrum
  plan(N, K, H, S)                                         (input items read, output floats written)

Plain module, no fixtures.
"""
import numpy as np

TOL = 1e-5  # conftest.relerr(got, ref) <= TOL: DESIGN.md "Tolerances"


def plan(N, K, H, S):
    return (0 if S == 0 else (S * K - 1) * H + N), S * N


def frames(x, N, K, H, S):
    """(S, K, N) view-like array of the frames of S spectra"""
    x = np.asarray(x).reshape(-1)
    assert x.size >= plan(N, K, H, S)[0]
    idx = (np.arange(S * K) * H)[:, None] + np.arange(N)[None, :]
    return x[idx].reshape(S, K, N)


def pspec64(x, N, K, H, S, window=None, shift=False, scale=1.0):
    if S == 0:
        return np.zeros((0, N))
    f = frames(x, N, K, H, S).astype(np.complex128)
    if window is not None:
        f = f * np.asarray(window, np.float64)
    X = np.fft.fft(f, axis=2)
    P = (X.real ** 2 + X.imag ** 2).sum(axis=1) * (float(scale) / K)
    return np.fft.fftshift(P, axes=1) if shift else P


def pspec(x, N, K, H, S, window=None, shift=False, log_output=False, scale=1.0):
    P = pspec64(x, N, K, H, S, window, shift, scale)
    if log_output:
        with np.errstate(divide="ignore"):
            P = 10.0 * np.log10(P)
    return P.astype(np.float32)


def hann(N):
    """periodic Hann, float32 as the block receives it"""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)


def make_input(n, seed=0):
    rng = np.random.default_rng(4000 + seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
