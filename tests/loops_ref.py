"""float64 restatement of clSignalSource and clCostasLoop (the fp64-device branch of lib/clSignalSource_impl.cc:113-237,386-399
and lib/clCostasLoop_impl.cc:165-226), numpy / python only.  Test infrastructure for tests/test_loops.py and test_loops_gpu.py;
the formulas are the ones stated in include/mi355_clenabled.h.

The signal source is vectorised.  The Costas loop is sequential in the item index and vectorised over streams (one numpy lane per
stream), so a few hundred streams cost what one costs; a long single stream goes through the scalar form, which is the same
arithmetic on python floats."""
import math

import numpy as np

TWO_PI = 6.28318530717958647692


def wrap(pos):
    """if (pos > 2pi || pos < -2pi) pos = (pos/2pi - (double)(int)(pos/2pi)) * 2pi"""
    if pos > TWO_PI or pos < -TWO_PI:
        r = pos / TWO_PI
        pos = (r - float(int(r))) * TWO_PI
    return pos


# ---------------------------------------------------------------------------------------------------------- signal source
def sig_inc(freq, samp_rate):
    return TWO_PI * float(freq) / float(samp_rate)


def sig_values(pos, inc, n, amplitude):
    """(cos d * A, sin d * A) in float64 for items 0 .. n-1 of a call starting at phase pos"""
    d = pos + inc * np.arange(n, dtype=np.float64)
    a = float(np.float32(amplitude))
    return np.cos(d) * a, np.sin(d) * a


def sig_advance(pos, inc, n):
    return wrap(pos + inc * float(np.float32(n)))


def sig_call(pos, inc, n, amplitude, dtype, waveform):
    """One call: (float64 values before the output conversion -- complex128 for dtype 'complex' --, phase after the call).
    dtype: 'complex', 'float' or 'int'; waveform 1 cos, 2 sin.  The int output is np.trunc of the values."""
    c, s = sig_values(pos, inc, n, amplitude)
    v = c + 1j * s if dtype == "complex" else (c if waveform == 1 else s)
    return v, sig_advance(pos, inc, n)


# ---------------------------------------------------------------------------------------------------------- Costas loop
def costas_gains(loop_bw):
    """gr::blocks::control_loop gains in float32 arithmetic -> (alpha, beta) as python floats"""
    f = np.float32
    bw = f(loop_bw)
    damp = f(np.sqrt(f(2.0))) / f(2.0)
    denom = f(1.0) + f(2.0) * damp * bw + bw * bw
    return float((f(4.0) * damp * bw) / denom), float((f(4.0) * bw * bw) / denom)


def costas(x, order, loop_bw, num_streams=1, state=None, trig_noise=0.0, rng=None):
    """x: complex64 [nitems * num_streams], item-major.  Returns (out complex128 [n*S] -- the doubles before the float rounding --,
    freq_out float64 [n*S], state = (phase[S], freq[S], error[S])).  trig_noise: relative noise put on every sin / cos (the
    stability check of the tests); state: start from (phase, freq, error) instead of zeros.  Where the kernel has an fma the
    product is rounded here before the sum: one double ulp, nothing a float output or a 1e-9 state comparison resolves."""
    S = int(num_streams)
    x = np.asarray(x).reshape(-1, S)
    n = x.shape[0]
    alpha, beta = costas_gains(loop_bw)
    if state is None:
        phase, freq, err = np.zeros(S), np.zeros(S), np.zeros(S)
    else:
        phase, freq, err = (np.array(v, dtype=np.float64).reshape(S).copy() for v in state)
    re_all, im_all = x.real.astype(np.float64), x.imag.astype(np.float64)
    out = np.empty((n, S), np.complex128)
    fo = np.empty((n, S), np.float64)
    for i in range(n):
        re, im = re_all[i], im_all[i]
        n_r, n_i = np.cos(-phase), np.sin(-phase)
        if trig_noise:
            n_r = n_r * (1.0 + trig_noise * rng.standard_normal(S))
            n_i = n_i * (1.0 + trig_noise * rng.standard_normal(S))
        o_r = re * n_r - im * n_i
        o_i = re * n_i + im * n_r
        out[i] = o_r + 1j * o_i
        if order == 2:
            e = o_r * o_i
        else:
            e = np.where(o_r > 0, 1.0, -1.0) * o_i - np.where(o_i > 0, 1.0, -1.0) * o_r
        e = 0.5 * (np.abs(e + 1.0) - np.abs(e - 1.0))
        freq = freq + beta * e
        phase = phase + (freq + alpha * e)
        big = (phase > TWO_PI) | (phase < -TWO_PI)
        if big.any():
            r = phase[big] / TWO_PI
            phase[big] = (r - np.trunc(r)) * TWO_PI
        freq = np.clip(freq, -1.0, 1.0)
        err = e
        fo[i] = freq
    return out.reshape(-1), fo.reshape(-1), (phase, freq, err)


def costas_scalar(x, order, loop_bw, state=None, trig_noise=0.0, rng=None):
    """The same recurrence for ONE stream on python floats (several times faster per item than the one-lane numpy form): for the
    long single-stream case."""
    alpha, beta = costas_gains(loop_bw)
    phase, freq, e = (0.0, 0.0, 0.0) if state is None else (float(state[0]), float(state[1]), float(state[2]))
    xr = np.asarray(x).real.astype(np.float64).tolist()
    xi = np.asarray(x).imag.astype(np.float64).tolist()
    n = len(xr)
    o_re, o_im, fo = [0.0] * n, [0.0] * n, [0.0] * n
    cos, sin = math.cos, math.sin
    noise = (1.0 + trig_noise * rng.standard_normal((n, 2))).tolist() if trig_noise else None
    for i in range(n):
        re, im = xr[i], xi[i]
        n_r, n_i = cos(-phase), sin(-phase)
        if noise:
            n_r, n_i = n_r * noise[i][0], n_i * noise[i][1]
        o_r = re * n_r - im * n_i
        o_i = re * n_i + im * n_r
        o_re[i], o_im[i] = o_r, o_i
        if order == 2:
            e = o_r * o_i
        else:
            e = (o_i if o_r > 0 else -o_i) - (o_r if o_i > 0 else -o_r)
        e = 0.5 * (abs(e + 1.0) - abs(e - 1.0))
        freq = freq + beta * e
        phase = phase + (freq + alpha * e)
        if phase > TWO_PI or phase < -TWO_PI:
            r = phase / TWO_PI
            phase = (r - float(int(r))) * TWO_PI
        freq = 1.0 if freq > 1.0 else (-1.0 if freq < -1.0 else freq)
        fo[i] = freq
    return np.array(o_re) + 1j * np.array(o_im), np.array(fo), (phase, freq, e)


def psk(rng, order, nitems, num_streams, sigma=0.05, max_offset=0.03):
    """Noisy PSK, item-major complex64 [nitems * num_streams]: per stream a frequency offset in +-max_offset rad/item and a random
    start phase.  Returns (x, offsets[S])."""
    S = int(num_streams)
    sym = rng.integers(0, order, size=(nitems, S))
    pts = np.exp(1j * (2 * np.pi * sym / order + (np.pi / 4 if order == 4 else 0.0)))
    off = rng.uniform(-max_offset, max_offset, S)
    ph0 = rng.uniform(-np.pi, np.pi, S)
    rot = np.exp(1j * (ph0[None, :] + off[None, :] * np.arange(nitems)[:, None]))
    noise = sigma * (rng.standard_normal((nitems, S)) + 1j * rng.standard_normal((nitems, S)))
    return (pts * rot + noise).astype(np.complex64).reshape(-1), off


# ---------------------------------------------------------------------------------------------------------- the cases of the tests
# Shared by tests/test_loops.py (which proves on the CPU that the restatement of every case is stable) and tests/test_loops_gpu.py.
LOOP_BW = 0.0628
COSTAS_ORDERS = (2, 4)
COSTAS_STREAMS = (1, 2, 3, 64, 65, 100, 256)
COSTAS_NITEMS = (1, 63, 64, 65, 1000, 4097)
COSTAS_LONG = (4, 1 << 18)     # (order, items) of the long single-stream case
_cache = {}


def costas_input(order, num_streams, nitems):
    """(x, offsets) of a grid case: the first nitems items of ONE 4097-item signal per (order, num_streams), so the cases of a
    stream count share their prefix."""
    key = ("in", order, num_streams)
    if key not in _cache:
        _cache[key] = psk(np.random.default_rng(1000 * order + num_streams), order, max(COSTAS_NITEMS), num_streams)
    x, off = _cache[key]
    return x[:nitems * num_streams], off


def costas_expected(order, num_streams, nitems):
    """(out, freq_out, state) of a grid case, computed once"""
    key = ("ref", order, num_streams, nitems)
    if key not in _cache:
        _cache[key] = costas(costas_input(order, num_streams, nitems)[0], order, LOOP_BW, num_streams)
    return _cache[key]


# the setter case of the GPU tests: 3 streams from a non-zero start state
COSTAS_START = (4, 3, 1000, (np.array([0.5, -1.0, 3.0]), np.array([0.01, -0.02, 0.0]), np.zeros(3)))


def costas_long_input():
    if "long" not in _cache:
        order, n = COSTAS_LONG
        _cache["long"] = psk(np.random.default_rng(77), order, n, 1)
    return _cache["long"]


def costas_long_expected():
    if "longref" not in _cache:
        _cache["longref"] = costas_scalar(costas_long_input()[0], COSTAS_LONG[0], LOOP_BW)
    return _cache["longref"]


# (order, streams, items per stream) of the smallest host call that runs three pieces: a piece of the host path is 2^21 items over all
# streams, here 32768 per stream, so two full pieces and one of three items
COSTAS_PIECES = (4, 64, 2 * 32768 + 3)


def costas_pieces_input():
    if "pieces" not in _cache:
        order, streams, n = COSTAS_PIECES
        _cache["pieces"] = psk(np.random.default_rng(78), order, n, streams)
    return _cache["pieces"]


def costas_pieces_expected():
    if "piecesref" not in _cache:
        order, streams, _ = COSTAS_PIECES
        _cache["piecesref"] = costas(costas_pieces_input()[0], order, LOOP_BW, streams)
    return _cache["piecesref"]


SIG_N = (1, 7, 64, 1000, 4099, 1 << 20)
SIG_RATIOS = (0.01234, -0.37, 0.5, 1e-7)      # freq / samp_rate
SIG_AMPS = (1.0, 1000.5)
SIG_SAMP_RATE = 48000.0
SIG_RAGGED = (1, 63, 500, 4099, 8192)
# int output: a truncation is only comparable away from the integers, so the int cases start at a phase off zero (sin 0 = 0 and
# A cos 0 = A are integers); from there the whole grid stays off them (tests/test_loops.py checks the cap for every case)
SIG_INT_PHASE = 0.7
SIG_INT_CASES = [(r, a, w) for r in SIG_RATIOS for a in SIG_AMPS for w in (1, 2)]
INT_EPS, INT_CAP = 1e-6, 1e-3


def near_integer(v):
    return np.abs(v - np.rint(v)) <= INT_EPS
