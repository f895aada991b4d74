"""Numpy float64 yardsticks of clFFT and clxcorrelate_fft_vcf for the sizes the oracle's O(N^2) DFT cannot run, and the per-frame error bounds
of clFFT (fft_frames64, fft_bound_check, the input kinds they are held on; DESIGN.md, 'Tolerances') and the per-frame, per-lag ones of the
correlator (xcorr_frames64, xcorr_bound_check).  Plain module (no fixtures), shared by tests/test_fft_gpu.py, tests/test_fft_bounds_gpu.py,
tests/test_xcorr_gpu.py, tests/test_xcorr_bounds_gpu.py and tests/switch_cases.py (whose child processes import no test module); the
transforms are tied to the oracle at small lengths in tests/test_fft_gpu.py and tests/test_xcorr_gpu.py, the multiples of the bounds are
fixed by tests/test_fft_ref.py and tests/test_xcorr_ref.py."""
import numpy as np


def fft_frames64(n, fwd, w, shift, x, real=False):
    """clFFT work() semantics (oracle/o_fft.c:140-188) on numpy's float64 pocketfft, NOT rounded to float: complex128, shape (frames, n).
    x: the float32 / complex64 items the block was given (real: float input, the imaginary part is zero); w: the window or None / []."""
    x = np.asarray(x)
    assert real == (not np.iscomplexobj(x)), "real says what the block's input type is"
    x = x.astype(np.complex128).reshape(-1, n)
    if w is not None and len(w):
        x = x * np.asarray(w, np.float64)
    if not fwd and shift:
        half = n // 2
        x = np.concatenate([x[:, half:], x[:, :half]], axis=1)  # original position i -> i + (n - half) for i < half
    y = np.fft.fft(x, axis=1) if fwd else np.fft.ifft(x, axis=1) * n
    if fwd and shift:
        ln = (n + 1) // 2
        y = np.concatenate([y[:, ln:], y[:, :ln]], axis=1)
    return y


def np_fft_block(n, fwd, w, shift, x):
    """fft_frames64 flattened and rounded to complex64: the oracle's O(N^2) DFT for lengths that are not a power of two cannot be run at
    10^5 .. 10^7 points.  Tied to the oracle at a small length in tests/test_fft_gpu.py."""
    x = np.asarray(x)
    return fft_frames64(n, fwd, w, shift, x, not np.iscomplexobj(x)).reshape(-1).astype(np.complex64)


# ---- per-frame error bounds of clFFT ('Tolerances'; the multiples are fixed by tests/test_fft_ref.py, never by a GPU result) ----
U32 = 2.0 ** -24
# (a, b): per bin and component  max(|Re d|, |Im d|) <= a u sqrt(L) S_f;  per frame  ||d_f||_2 <= b u sqrt(L) E_f
FFT_MULT = {"direct": (4.0, 3.0), "chirpz": (8.0, 4.0), "mixed_radix": (13.0, 8.0), "mixed_radix_two_passes": (11.0, 6.0)}
# The mixed-radix routes form the twiddles W^r of a butterfly (r < radix <= 16) from ONE table entry W: W^2, W^4, W^8 by squaring, W^r by up to
# three further products (and the two-pass form its W_N^(n2 k1) the same way, from a base and a step entry): more roundings by
# construction, so these routes have multiples of their own, fixed on complex64 emulations of exactly these pass structures: each is the
# smallest integer at or above twice the largest figure the emulation reaches (6.01 / 3.64 units in one pass, 5.11 / 2.77 in two), which is
# the half rule and nothing more.
# The plans (radices per pass, the rule's factorisation first and the alternative one where it differs; two passes: n1, n2 and the radices of
# either) of every such length the GPU tests use: tests/test_fft_ref.py emulates each, and a case of tests/test_fft_bounds_gpu.py whose
# last_route() names another plan fails.
MR_PLANS = {
    6: [(3, 2)], 12: [(3, 4)], 14: [(7, 2)], 15: [(5, 3)], 21: [(7, 3)], 22: [(11, 2)], 35: [(7, 5)], 48: [(3, 16)], 56: [(7, 8)],
    81: [(9, 9), (3, 3, 3, 3)], 96: [(12, 8), (3, 8, 4)], 100: [(10, 10), (5, 5, 4)], 105: [(15, 7)], 112: [(14, 8)], 120: [(15, 8)],
    143: [(13, 11)], 144: [(12, 12), (3, 3, 16)], 196: [(14, 14)], 200: [(5, 5, 8)], 210: [(15, 14)], 360: [(15, 3, 8)], 675: [(15, 15, 3)],
    729: [(9, 9, 9), (3, 3, 3, 3, 3, 3)], 1000: [(10, 10, 10), (5, 5, 5, 8)], 1100: [(11, 10, 10)], 1125: [(15, 15, 5)], 1331: [(11, 11, 11)],
    1536: [(12, 16, 8), (3, 8, 8, 8)], 1715: [(7, 7, 7, 5)], 1728: [(12, 12, 12), (3, 3, 3, 8, 8)], 2000: [(5, 5, 5, 16)], 2197: [(13, 13, 13)],
    2400: [(15, 10, 16), (15, 5, 8, 4)], 2401: [(7, 7, 7, 7)], 2744: [(14, 14, 14)], 2860: [(13, 11, 5, 4)], 3000: [(15, 5, 5, 8)],
    3375: [(15, 15, 15)], 3584: [(14, 16, 16)], 3840: [(15, 16, 16)], 4000: [(10, 10, 5, 8), (5, 5, 5, 8, 4)], 4095: [(15, 13, 7, 3)],
    4200: [(15, 7, 5, 8)], 5000: [(10, 10, 10, 5), (5, 5, 5, 5, 8)], 5625: [(15, 15, 5, 5)], 6000: [(15, 5, 5, 16)], 7168: [(14, 8, 8, 8)],
    7680: [(15, 8, 8, 8)], 9000: [(15, 15, 5, 8)], 10000: [(10, 10, 10, 10), (5, 5, 5, 5, 16)], 11264: [(11, 16, 8, 8)], 12000: [(15, 5, 5, 8, 4)],
    12005: [(7, 7, 7, 7, 5)], 13312: [(13, 16, 8, 8)], 14336: [(14, 16, 8, 8)], 15000: [(15, 5, 5, 5, 8)], 15360: [(15, 16, 8, 8)],
}
MR_TILE_PLANS = {
    16000: (100, 160, (10, 10), (10, 16)), 20000: (125, 160, (5, 5, 5), (10, 16)), 22050: (105, 210, (15, 7), (15, 14)),
    30030: (165, 182, (15, 11), (14, 13)), 44100: (210, 210, (15, 14), (15, 14)), 48000: (200, 240, (5, 5, 8), (15, 16)),
    50625: (225, 225, (15, 15), (15, 15)), 100000: (250, 400, (10, 5, 5), (5, 5, 16)), 250000: (500, 500, (10, 10, 5), (10, 10, 5)),
    921600: (960, 960, (15, 8, 8), (15, 8, 8)),
}


def fft_unit(n):
    """u sqrt(L), L = ceil(log2 n): the rounding error of a float32 FFT relative to its largest intermediate magnitude"""
    return U32 * np.sqrt(float(int(n - 1).bit_length()))


def fft_bound_check(got, ref64, n, kind="direct", check=True, what=""):
    """Every frame f of got (complex64 items, any shape) against the float64 reference (fft_frames64), with S_f = max_k |X_f[k]| and
    E_f = ||X_f||_2 of the reference:
        per bin and component   max(|Re d|, |Im d|) <= a u sqrt(L) S_f
        per frame               ||d_f||_2          <= b u sqrt(L) E_f
        zero frame              S_f == 0: got is exactly zero there
    (a, b) = FFT_MULT[kind].  Returns the largest used fraction of each bound (bin, rss); check = True asserts both <= 1 and the zero
    frames; check = False only measures (the planted errors of tests/test_fft_ref.py, the checks of tests/switch_cases.py) and returns inf for
    both when a frame of zeros did not come out as zeros."""
    a, b = FFT_MULT[kind]
    ref = np.asarray(ref64).reshape(-1, n)
    assert ref.dtype == np.complex128, "the reference is the float64 one, not a rounded result"
    got = np.asarray(got).reshape(-1, n)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    unit = fft_unit(n)
    mag = np.abs(ref)
    S = mag.max(axis=1)
    E = np.sqrt((mag * mag).sum(axis=1))
    d = got - ref  # complex128; a non-finite got gives a non-finite d, which fails every comparison below
    dbin = np.maximum(np.abs(d.real), np.abs(d.imag)).max(axis=1)
    drss = np.sqrt((d.real * d.real + d.imag * d.imag).sum(axis=1))
    zero = S == 0
    zero_ok = bool(np.all(got[zero] == 0))
    live = ~zero
    with np.errstate(invalid="ignore", divide="ignore"):
        fb = dbin[live] / (a * unit * S[live])
        fr = drss[live] / (b * unit * E[live])
    fb = np.where(np.isfinite(fb), fb, np.inf)
    fr = np.where(np.isfinite(fr), fr, np.inf)
    frac_bin = float(fb.max()) if fb.size else 0.0
    frac_rss = float(fr.max()) if fr.size else 0.0
    if not zero_ok and not check:
        return float("inf"), float("inf")
    if check:
        live_idx = np.flatnonzero(live)
        assert zero_ok, "%s: a frame of zeros did not come out as zeros (frames %s)" % (what, np.flatnonzero(zero & (np.abs(got).max(axis=1) != 0))[:8])
        assert frac_bin <= 1.0, "%s: per-bin bound used %.3g times over (frame %d, n %d, %s)" % (what, frac_bin, live_idx[int(fb.argmax())], n, kind)
        assert frac_rss <= 1.0, "%s: per-frame bound used %.3g times over (frame %d, n %d, %s)" % (what, frac_rss, live_idx[int(fr.argmax())], n, kind)
    return frac_bin, frac_rss


def fft_bound_kind(route):
    """the multiples a result is held to, from clFFT.last_route() of the call that made it"""
    if route.startswith("k_fft_mr_tile "):
        return "mixed_radix_two_passes"
    if route.startswith("k_fft_mr "):
        return "mixed_radix"
    if route.startswith(("k_chirpz<", "bluestein ")):
        return "chirpz"
    assert route.startswith("k_fft"), "no clFFT route: %r" % route
    return "direct"


def fft_held(got, route, n, fwd, w, shift, x, what=""):
    """fft_bound_check of a call's output against the float64 transform of its input x (float32: real input), with the multiples of the
    route that ran: for the call sites that hold an input and a float32 reference (the golden vectors), or a relerr comparison"""
    x = np.asarray(x)
    ref = fft_frames64(n, fwd, w, shift, x, not np.iscomplexobj(x))
    return fft_bound_check(got, ref, n, fft_bound_kind(route), what="%s %s" % (route, what))


def fft_inputs(kind, n, frames, seed, real=False):
    """The input kinds the bounds are held on, `frames` frames of n items (complex64, or float32 when real), shape (frames, n):
    mixed      noise frames scaled by 10^U(-3, 3) per frame; frames[-1] (frames >= 3) and frames[frames // 2] (frames >= 5) are all zero
    impulses   frame j has a unit impulse at position impulse_positions(n, frames)[j]
    tones      frame j is exp(2 pi i k_j t / n) (cos for real input) at bin tone_bins(n, frames)[j], built in float64 and rounded
    tone_noise the tones plus noise 60 dB below them"""
    rng = np.random.default_rng(seed)

    def noise(shape):
        v = rng.standard_normal(shape)
        return v if real else v + 1j * rng.standard_normal(shape)

    if kind == "mixed":
        x = noise((frames, n)) * 10.0 ** rng.uniform(-3.0, 3.0, (frames, 1))
        if frames >= 3:
            x[-1] = 0
        if frames >= 5:  # (a three-frame case keeps two live frames of different scale)
            x[frames // 2] = 0
    elif kind == "impulses":
        x = np.zeros((frames, n), np.float64 if real else np.complex128)
        x[np.arange(frames), impulse_positions(n, frames)] = 1.0
    elif kind in ("tones", "tone_noise"):
        ph = 2.0 * np.pi * np.outer(tone_bins(n, frames), np.arange(n)) / n
        x = np.cos(ph) if real else np.exp(1j * ph)
        if kind == "tone_noise":
            x = x + 1e-3 * noise((frames, n))
    else:
        raise ValueError(kind)
    return x.astype(np.float32 if real else np.complex64)


def _edge_then_seeded(n, count, edges, seed):
    """count values in [0, n): the edge values first (those below n, once each), then seeded ones"""
    out = []
    for v in edges:
        if 0 <= v < n and v not in out:
            out.append(v)
    rng = np.random.default_rng(seed)
    while len(out) < count:
        out.append(int(rng.integers(0, n)))
    return np.asarray(out[:count], np.int64)


def impulse_positions(n, frames):
    """frames >= n: the identity first (every position once: the outputs are the whole DFT matrix), then seeded ones; else 1, n/2-1, n/2, n-1, 0 (a one-frame case gets position 1, whose transform is W_n^k itself), then seeded ones"""
    if frames >= n:
        return np.concatenate([np.arange(n), _edge_then_seeded(n, frames - n, (), 1000 + n)])
    return _edge_then_seeded(n, frames, (1, n // 2 - 1, n // 2, n - 1, 0), 1000 + n)


def tone_bins(n, frames):
    """frames >= n: every bin once, then seeded ones; else 1, n/2, n-1, 0, then seeded ones"""
    if frames >= n:
        return np.concatenate([np.arange(n), _edge_then_seeded(n, frames - n, (), 2000 + n)])
    return _edge_then_seeded(n, frames, (1, n // 2, n - 1, 0), 2000 + n)


def xcorr_frames64(n, itype, ins):
    """clxcorrelate_fft_vcf's definition on numpy's float64 pocketfft, NOT rounded to float.  ins: the complex64 items the block was given
    (input 0 the reference).  For every signal s >= 1: (|r| with the two halves of every vector exchanged, float64, shape (frames, n);
    (T, S)), r = ifft(X0 conj(Xs)) n, X = the input (itype 1, spectra) or its forward transform (itype 2, time series), and the per-frame
    scales of xcorr_bound_check: T_f = ||P_f||_2 of P = X0 conj(Xs), plus sqrt(n) ||x0_f||_2 ||xs_f||_2 for time series; S_f = max_m |r_f[m]|."""
    x = [np.asarray(v).astype(np.complex128).reshape(-1, n) for v in ins]
    spec = x if itype == 1 else [np.fft.fft(v, axis=1) for v in x]
    e = [np.sqrt((v.real * v.real + v.imag * v.imag).sum(axis=1)) for v in x]
    outs = []
    for s in range(1, len(x)):
        P = spec[0] * np.conj(spec[s])
        r = np.abs(np.fft.ifft(P, axis=1) * n)
        T = np.sqrt((P.real * P.real + P.imag * P.imag).sum(axis=1))
        if itype != 1:
            T = T + np.sqrt(float(n)) * e[0] * e[s]
        outs.append((np.concatenate([r[:, n // 2:], r[:, :n // 2]], axis=1), (T, r.max(axis=1))))
    return outs


def np_xcorr(n, itype, ins):
    """xcorr_frames64 flattened and rounded to float (the oracle's O(N^2) DFT cannot run lengths that are not a power of two at these
    sizes); tied to the oracle at a small length in tests/test_xcorr_gpu.py."""
    return [mag.reshape(-1).astype(np.float32) for mag, _ in xcorr_frames64(n, itype, ins)]


# ---- per-frame, per-lag error bounds of clxcorrelate_fft_vcf ('Tolerances'; the multiples are fixed by tests/test_xcorr_ref.py,
# never by a GPU result).  (a, b): per lag  |d| <= a unit (T_f + S_f);  per frame  ||d_f||_2 <= b unit sqrt(n) T_f.  Keyed by the clFFT
# route kind of the transforms underneath (fft_bound_kind): `direct` is the fused kernel and the composed route over power-of-two transforms ----
# Each is the smallest integer at or above twice the largest figure of the CPU evaluations of that structure: 1.34 / 1.81 units (radix 2 and
# pocketfft), 2.20 / 1.92 (chirp-z), 2.92 / 3.02 (mixed radix, one pass: the twiddle products), 2.74 / 1.93 (two passes).
XCORR_MULT = {"direct": (3.0, 4.0), "chirpz": (5.0, 4.0), "mixed_radix": (6.0, 7.0), "mixed_radix_two_passes": (6.0, 4.0)}


def xcorr_unit(n, itype):
    """u sqrt(L) for spectra (one transform), u sqrt(2 L) for time series (two transforms in series), L = ceil(log2 n)"""
    L = float(int(n - 1).bit_length())
    return U32 * np.sqrt(L if itype == 1 else 2.0 * L)


def xcorr_bound_check(got, ref, scales, n, itype, kind="direct", check=True, what=""):
    """Every frame f of one output of the correlator (float32 items, any shape) against xcorr_frames64's (|r|, (T, S)) of that signal:
        per lag      |got - |r||         <= a unit (T_f + S_f)
        per frame    ||got_f - |r_f|||_2 <= b unit sqrt(n) T_f
        zero frame   T_f == 0 (either operand's frame all zero; for spectra also disjoint supports): got is exactly zero there
        non-finite   a non-finite got fails
    unit = xcorr_unit(n, itype), (a, b) = XCORR_MULT[kind].  T_f is the size of what the inverse transform is given (its rounding error is
    unit T_f per lag whatever the result sums to) and, for time series, of what the forward transforms' error leaves in the product (which
    does not shrink when P cancels, as for orthogonal tones); S_f covers the coherent peak, whose own rounding (the magnitude, the last
    butterflies) is relative to it.  Returns the largest used fraction of each bound (lag, frame); check = True asserts both <= 1 and the
    zero frames; check = False only measures and returns inf for both when a zero frame did not come out as zeros."""
    a, b = XCORR_MULT[kind]
    ref = np.asarray(ref).reshape(-1, n)
    assert ref.dtype == np.float64, "the reference is the float64 one, not a rounded result"
    got = np.asarray(got).reshape(-1, n).astype(np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    T, S = (np.asarray(v, np.float64) for v in scales)
    unit = xcorr_unit(n, itype)
    d = np.abs(got - ref)  # a non-finite got gives a non-finite d, which fails every comparison below
    dlag = d.max(axis=1)
    drss = np.sqrt((d * d).sum(axis=1))
    zero = T == 0
    zero_ok = bool(np.all(got[zero] == 0))
    live = ~zero
    with np.errstate(invalid="ignore", divide="ignore"):
        fl = dlag[live] / (a * unit * (T[live] + S[live]))
        fr = drss[live] / (b * unit * np.sqrt(float(n)) * T[live])
    fl = np.where(np.isfinite(fl), fl, np.inf)
    fr = np.where(np.isfinite(fr), fr, np.inf)
    frac_lag = float(fl.max()) if fl.size else 0.0
    frac_rss = float(fr.max()) if fr.size else 0.0
    if not zero_ok and not check:
        return float("inf"), float("inf")
    if check:
        live_idx = np.flatnonzero(live)
        assert zero_ok, "%s: a zero frame did not come out as zeros (frames %s)" % (what, np.flatnonzero(zero & ~((got == 0).all(axis=1)))[:8])
        assert frac_lag <= 1.0, "%s: per-lag bound used %.3g times over (frame %d, n %d, %s)" % (what, frac_lag, live_idx[int(fl.argmax())], n, kind)
        assert frac_rss <= 1.0, "%s: per-frame bound used %.3g times over (frame %d, n %d, %s)" % (what, frac_rss, live_idx[int(fr.argmax())], n, kind)
    return frac_lag, frac_rss


def xcorr_held(outs, n, itype, ins, kind="direct", what=""):
    """xcorr_bound_check of every output of a call against the float64 definition of its inputs: for the call sites that hold a relerr
    comparison.  Returns the largest used fractions (lag, frame) over the outputs."""
    used = [xcorr_bound_check(o, mag, sc, n, itype, kind, what="%s output %d" % (what, k))
            for k, (o, (mag, sc)) in enumerate(zip(outs, xcorr_frames64(n, itype, ins)))]
    return max(u[0] for u in used), max(u[1] for u in used)

