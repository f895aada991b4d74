"""GPU: clxcorrelate_fft_vcf held to the per-frame, per-lag bounds of tests/fft_ref.py (xcorr_bound_check against the float64 definition
xcorr_frames64; the multiples are fixed on the CPU by tests/test_xcorr_ref.py), to known answers, to independence of a result from the other
frames and signals of its call, and to frame-local reach (include/mi355_clenabled.h states the contract).

Every call runs work_device into outputs filled with NaN.  Inputs (fft_ref.fft_inputs): `mixed` -- noise frames scaled by 10^U(-3, 3) per
frame with two all-zero frames, one of them the last frame of the ragged last group; `impulses`, `tones` -- the identity / one tone per bin
where the call has that many frames, edge and seeded positions otherwise; `tone_noise` -- the tones plus noise at -60 dB.  Every product of
two frames has a scale of its own, 10^-6 ... 10^6 in a `mixed` pair, which is what one scale per call (relerr) cannot see.

The fused kernel (powers of two 16 ... 4096) owns F = 4096 / n frames per workgroup: frames = max(2 F + 1, 9) is two full groups and a ragged
one.  The composed route (every other even length) is run once per clFFT route underneath, at the smallest even length that takes it; the
route is read from a clFFT of that length (switch_cases.xcorr_route_kind) and picks the multiples.

Every test prints `USED <route> ...` lines with the used fraction of each bound (pytest -s); DESIGN.md, 'Tolerances', records them."""
import numpy as np
import pytest
import torch

from conftest import GPU_ARGS
from fft_ref import XCORR_MULT, fft_inputs, xcorr_bound_check, xcorr_frames64, xcorr_unit
from switch_cases import xcorr_route_kind
from test_device_bounds_gpu import ALL4, _run_offsets

pytestmark = pytest.mark.gpu

KINDS = ["mixed", "impulses", "tones", "tone_noise"]
FUSED = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
ITYPES = [pytest.param(1, id="spectra"), pytest.param(2, id="time_series")]


def _blk(gpu, n, nin, itype):
    ocl, sel, plat, dev = GPU_ARGS
    return gpu.clxcorrelate_fft_vcf(n, nin, ocl, sel, plat, dev, itype)


def _frames(n):
    return max(2 * (4096 // n) + 1, 9)


def _dev(x):
    """(frames, n) complex64 -> (frames, n, 2) float on the device"""
    return torch.view_as_real(torch.from_numpy(np.ascontiguousarray(x)).cuda()).contiguous()


def _call(blk, frames, n, d_ins):
    outs = [torch.full((frames, n), float("nan"), device="cuda") for _ in d_ins[1:]]
    blk.work_device(frames, d_ins, outs)
    torch.cuda.synchronize()
    return outs


def _run(blk, frames, n, ins):
    return [o.cpu().numpy() for o in _call(blk, frames, n, [_dev(x) for x in ins])]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _hold(outs, n, itype, ins, kind, label):
    """every output against the float64 definition: prints the used fractions, then asserts; returns the references"""
    refs = xcorr_frames64(n, itype, ins)
    for k, (o, (mag, sc)) in enumerate(zip(outs, refs)):
        fl, fr = xcorr_bound_check(o, mag, sc, n, itype, kind, check=False)
        print("USED %s output %d: lag %.3f frame %.3f" % (label, k, fl, fr))
    for k, (o, (mag, sc)) in enumerate(zip(outs, refs)):
        xcorr_bound_check(o, mag, sc, n, itype, kind, what="%s output %d" % (label, k))
    return refs


# ------------------------------------------------------------------------------------------------------------ fused kernel: bounds

@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n", FUSED)
def test_fused_kernel_holds_the_bounds_on_all_sixteen_pairs(gpu, n, itype):
    """five inputs: input 0 one kind, inputs 1 .. 4 the four kinds; four calls.  A zero frame in only one operand: (mixed, tones), (tones, mixed)"""
    frames = _frames(n)
    blk = _blk(gpu, n, 5, itype)
    sigs = [fft_inputs(k, n, frames, 11 * n + 1 + i) for i, k in enumerate(KINDS)]
    for j, k0 in enumerate(KINDS):
        ins = [fft_inputs(k0, n, frames, 13 * n + 100 + j)] + sigs
        outs = _run(blk, frames, n, ins)
        _hold(outs, n, itype, ins, "direct", "k_xcorr<%d> %s frames %d %s x (%s)" % (n, "spectra" if itype == 1 else "time series", frames, k0, ", ".join(KINDS)))


# ------------------------------------------------------------------------------------------------------------------- known answers

@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n", FUSED)
def test_autocorrelation_peaks_at_the_middle_with_the_frame_energy(gpu, n, itype):
    """signal = reference: lag 0 sits at index n / 2 and is sum_k |X_f[k]|^2 (time series: n ||x_f||^2) within the per-lag bound; once with
    two separate copies of the data, once with the SAME tensor given as both inputs"""
    frames = _frames(n)
    x = fft_inputs("mixed", n, frames, 17 * n + itype)
    blk = _blk(gpu, n, 2, itype)
    d0 = _dev(x)
    (two,), (one,) = _call(blk, frames, n, [d0, d0.clone()]), _call(blk, frames, n, [d0, d0])
    assert torch.equal(_bits(two), _bits(one)), "the same tensor as both inputs gives other bits than two copies of it"
    got = two.cpu().numpy()
    ((mag, (T, S)),) = _hold([got], n, itype, [x, x], "direct", "k_xcorr<%d> autocorrelation %s" % (n, "spectra" if itype == 1 else "time series"))
    x64 = x.astype(np.complex128)
    energy = (x64.real ** 2 + x64.imag ** 2).sum(axis=1) * (n if itype == 2 else 1)
    a = XCORR_MULT["direct"][0]
    live = T > 0
    assert live.sum() == frames - 2
    assert np.all(np.abs(got[:, n // 2] - energy)[live] <= (a * xcorr_unit(n, itype) * (T + S))[live])
    assert np.all(got.argmax(axis=1)[live] == n // 2)


@pytest.mark.parametrize("n", FUSED)
def test_delayed_copy_peaks_at_its_lag_in_every_frame(gpu, n):
    """time series under mixed per-frame scales: a copy delayed by d peaks at lag -d, which the half swap puts at (n / 2 - d) mod n, in
    every live frame -- the quiet ones as well"""
    frames, d = _frames(n), n // 3
    x = fft_inputs("mixed", n, frames, 19 * n)
    xs = np.roll(x, d, axis=1)
    (got,) = _run(_blk(gpu, n, 2, 2), frames, n, [x, xs])
    ((mag, (T, S)),) = _hold([got], n, 2, [x, xs], "direct", "k_xcorr<%d> delayed copy" % n)
    live = T > 0
    assert np.all(mag.argmax(axis=1)[live] == (n // 2 - d) % n)  # (the definition itself)
    assert np.all(got.argmax(axis=1)[live] == (n // 2 - d) % n)


# ----------------------------------------------------------------------------------------------------------------------- 32 inputs

@pytest.mark.parametrize("n,itype", [(16, 2), (128, 2), (4096, 2), (128, 1)], ids=["16-time_series", "128-time_series", "4096-time_series", "128-spectra"])
def test_thirty_two_inputs_equal_thirty_one_two_input_calls(gpu, n, itype):
    """the maximum the block takes (512 bytes of kernel arguments): every output inside the bounds, and output s - 1 bit for bit what a
    two-input block makes of (input 0, input s) -- a signal's result does not depend on the signals before it in the loop"""
    frames = 4096 // n + 1
    ins = [fft_inputs("mixed", n, frames, 23 * n)] + [fft_inputs(KINDS[s % 4], n, frames, 23 * n + s) for s in range(1, 32)]
    d_ins = [_dev(x) for x in ins]
    outs = _call(_blk(gpu, n, 32, itype), frames, n, d_ins)
    refs = xcorr_frames64(n, itype, ins)
    used = [xcorr_bound_check(o.cpu().numpy(), mag, sc, n, itype, "direct", what="32 inputs, output %d" % k) for k, (o, (mag, sc)) in enumerate(zip(outs, refs))]
    print("USED k_xcorr<%d> 32 inputs %s: lag %.3f frame %.3f" % (n, "spectra" if itype == 1 else "time series", max(u[0] for u in used), max(u[1] for u in used)))
    pair = _blk(gpu, n, 2, itype)
    for s in range(1, 32):
        (alone,) = _call(pair, frames, n, [d_ins[0], d_ins[s]])
        assert torch.equal(_bits(alone), _bits(outs[s - 1])), "output %d of the 32-input call differs from the two-input call" % (s - 1)


# ------------------------------------------------------------------------------------------------------------------ frame position

@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n", [16, 128, 1024])
def test_a_frame_alone_has_the_bits_it_has_inside_a_call(gpu, n, itype):
    """frames from the middle and the end of a 2 F + 1 call (the ragged group), and the first, run again alone with nframes = 1"""
    F = 4096 // n
    frames = 2 * F + 1
    ins = [fft_inputs(k, n, frames, 29 * n + i) for i, k in enumerate(("mixed", "tone_noise", "mixed"))]
    ins[0][-1], ins[0][frames // 2] = ins[1][0], ins[1][1]  # (the frames picked below are live)
    d_ins = [_dev(x) for x in ins]
    blk = _blk(gpu, n, 3, itype)
    whole = _call(blk, frames, n, d_ins)
    for f in (0, F - 1, frames // 2, 2 * F - 1, frames - 1):
        alone = _call(blk, 1, n, [d[f:f + 1].clone() for d in d_ins])
        for k in range(2):
            assert torch.isfinite(alone[k]).all()
            assert torch.equal(_bits(alone[k][0]), _bits(whole[k][f])), "frame %d of output %d depends on its position in the call" % (f, k)


# ---------------------------------------------------------------------------------------------------------------------------- reach

@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n", [16, 128, 1024, 4096, 1000])
def test_reach_is_the_frame_and_the_signal(gpu, n, itype):
    """three inputs; NaN in both components of the first item of frame 1 of input 1, the last item of a middle frame of input 0 and item
    n / 3 of the last frame (the ragged group) of input 2.  A plant in input s >= 1 makes every lag of that frame of output s - 1
    non-finite, a plant in input 0 that frame of every output; every other frame of every output keeps the bits of the clean call"""
    fused = n & (n - 1) == 0
    frames = _frames(n) if fused else 7
    d_ins = [_dev(fft_inputs("mixed", n, frames, 31 * n + s)) for s in range(3)]
    blk = _blk(gpu, n, 3, itype)
    clean = _call(blk, frames, n, d_ins)
    assert all(bool(torch.isfinite(c).all()) for c in clean)
    mid = frames // 2 + 1
    plants = [(1, 1, 0), (0, mid, n - 1), (2, frames - 1, n // 3)]  # (input, frame, item)
    dirty = [d.clone() for d in d_ins]
    for s, f, i in plants:
        dirty[s][f, i] = float("nan")
    got = _call(blk, frames, n, dirty)
    for k in range(2):
        hit = sorted({f for s, f, _ in plants if s in (0, k + 1)})
        assert len(hit) == 2
        bad = ~torch.isfinite(got[k])
        for f in hit:
            assert bool(bad[f].all()), "output %d: a non-finite item in frame %d left %d lags of it finite" % (k, f, int((~bad[f]).sum()))
        same = (_bits(got[k]) == _bits(clean[k])).all(dim=1)
        same[hit] = True
        wrong = torch.nonzero(~same).flatten()
        assert wrong.numel() == 0, "output %d: non-finite items in frames %s changed frames %s" % (k, hit, wrong[:8].tolist())


# ---------------------------------------------------------------------------------------------------------------------- guard bands

@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n", [16, 128, 4096])
def test_stays_inside_its_buffers_and_holds_the_bounds(gpu, n, itype):
    """16 and 128 points: the staged load and the staged float store; a ragged frame count; input and output 0 and 1 item past a 16-byte
    boundary in the four combinations; NaN around the inputs, a sentinel around the outputs, the interior held to the bounds"""
    frames = _frames(n)
    blk = _blk(gpu, n, 3, itype)
    ins = [fft_inputs(k, n, frames, 37 * n + i) for i, k in enumerate(("mixed", "mixed", "tone_noise"))]
    refs = xcorr_frames64(n, itype, ins)
    used = []

    def check(outs):
        used.extend(xcorr_bound_check(o, mag, sc, n, itype, "direct", what="output %d" % k) for k, (o, (mag, sc)) in enumerate(zip(outs, refs)))

    _run_offsets(lambda i, o: blk.work_device(frames, i, o), [(x, n) for x in ins], [(frames * n, np.float32, n)] * 2, ALL4, check, False)
    print("USED k_xcorr<%d> guard bands %s: lag %.3f frame %.3f" % (n, "spectra" if itype == 1 else "time series", max(u[0] for u in used), max(u[1] for u in used)))


# -------------------------------------------------------------------------------------------------------------------- composed route

COMPOSED = [(2, {}), (8, {}), (8192, {}), (32768, {}), (65536, {}), (12, {}), (3840, {}), (1000, {"MI355_FFT_MR_VARIANT": "0"}),
            (1000, {"MI355_FFT_MR_VARIANT": "1"}), (16000, {}), (2 * 2053, {}), (2 * 4099, {}), (1 << 21, {})]


@pytest.mark.parametrize("itype", ITYPES)
@pytest.mark.parametrize("n,env", COMPOSED, ids=["%d%s" % (n, "".join("-%s=%s" % (k.replace("MI355_FFT_", ""), v) for k, v in e.items())) for n, e in COMPOSED])
def test_composed_route_holds_the_bounds_of_the_clfft_route_underneath(gpu, monkeypatch, n, env, itype):
    """three inputs, `mixed` against `mixed` and `tone_noise`; 7 frames below 5000 points, 2 above; 2^21 points: one frame, two inputs, both kinds in turn"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kind, route = xcorr_route_kind(gpu, n)
    label = "composed | %s | n %d %s" % (route, n, "spectra" if itype == 1 else "time series")
    if n == 1 << 21:
        blk = _blk(gpu, n, 2, itype)
        x0 = fft_inputs("mixed", n, 1, 41)
        for i, k1 in enumerate(("mixed", "tone_noise")):
            ins = [x0, fft_inputs(k1, n, 1, 42 + i)]
            _hold(_run(blk, 1, n, ins), n, itype, ins, kind, "%s mixed x %s" % (label, k1))
        return
    frames = 7 if n < 5000 else 2
    ins = [fft_inputs(k, n, frames, 41 * n + i) for i, k in enumerate(("mixed", "mixed", "tone_noise"))]
    _hold(_run(_blk(gpu, n, 3, itype), frames, n, ins), n, itype, ins, kind, label + " frames %d" % frames)


# ------------------------------------------------------------------------------------------------------------------------ host path

@pytest.mark.parametrize("itype", ITYPES)
def test_host_path_equals_the_device_path(gpu, itype):
    n, frames = 256, 37
    ins = [fft_inputs(k, n, frames, 43 + i) for i, k in enumerate(("mixed", "tone_noise", "mixed"))]
    blk = _blk(gpu, n, 3, itype)
    dev = _run(blk, frames, n, ins)
    host = [np.full(frames * n, np.nan, np.float32) for _ in range(2)]
    assert blk.work(frames, [x.reshape(-1) for x in ins], host) == frames
    for k in range(2):
        assert np.array_equal(host[k].view(np.int32), dev[k].reshape(-1).view(np.int32)), "output %d: work() and work_device differ" % k
    _hold(host, n, itype, ins, "direct", "k_xcorr<256> host path %s" % ("spectra" if itype == 1 else "time series"))
