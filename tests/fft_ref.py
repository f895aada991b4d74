"""Numpy float64 yardsticks of clFFT and clxcorrelate_fft_vcf for the sizes the oracle's O(N^2) DFT cannot run.  Plain module (no fixtures), shared
by tests/test_fft_gpu.py, tests/test_xcorr_gpu.py and tests/switch_cases.py (whose child processes import no test module); both functions are
tied to the oracle at small lengths in those two test files."""
import numpy as np


def np_fft_block(n, fwd, w, shift, x):
    """clFFT work() semantics (oracle/o_fft.c:140-188) on numpy's float64 pocketfft: the oracle's O(N^2) DFT for lengths that are not a
    power of two cannot be run at 10^5 .. 10^7 points.  Tied to the oracle at a small length in the test below."""
    x = x.astype(np.complex128).reshape(-1, n)
    if w is not None:
        x = x * np.asarray(w, np.float64)
    if not fwd and shift:
        half = n // 2
        x = np.concatenate([x[:, half:], x[:, :half]], axis=1)  # original position i -> i + (n - half) for i < half
    y = np.fft.fft(x, axis=1) if fwd else np.fft.ifft(x, axis=1) * n
    if fwd and shift:
        ln = (n + 1) // 2
        y = np.concatenate([y[:, ln:], y[:, :ln]], axis=1)
    return y.reshape(-1).astype(np.complex64)


def np_xcorr(n, itype, ins):
    """The block's definition on numpy's float64 pocketfft (the oracle's O(N^2) DFT cannot run lengths that are not a power of two
    at these sizes); tied to the oracle at a small length in the test below."""
    x = [v.astype(np.complex128).reshape(-1, n) for v in ins]
    spec = x if itype == 1 else [np.fft.fft(v, axis=1) for v in x]
    outs = []
    for sp in spec[1:]:
        r = np.abs(np.fft.ifft(spec[0] * np.conj(sp), axis=1) * n)
        outs.append(np.concatenate([r[:, n // 2:], r[:, :n // 2]], axis=1).reshape(-1).astype(np.float32))
    return outs
