"""GPU: clFEngine against tests/fengine_ref.py (float64 numpy).  Every device call runs on guard-banded buffers (tests/guarded.py); the
output interior holds -128 before the call, a value the block never produces, so a byte the call did not write shows.

Routes, as csrc/fengine.hip states them:
  fused    F = 16 .. 4096 a power of two, P <= 16: k_fengine<F, npol>
  generic  every other F, P > 16, and every handle under set_generic(True): k_fe_woa + clFFT + k_fe_quant

Exact pins compare with array_equal.  Random data compare with the float64 reference where the reference's value is further than delta
from every decision boundary of the quantiser; delta is the float32 error bound derived in tests/fengine_ref.py from the inputs, the
taps and the gains alone (8 sigma of the root-sum-square model written down there).  Elsewhere either neighbour is accepted; each random
case asserts that those components are at most 1 % and prints the share and the number of components that differed.

On an MI355X the file takes 3.6 s (37 tests); delta stayed below 7.2e-4, the exempted share below 0.11 %, and at most one component of a
case differed from the reference (31 of the 8.7 million of the 16384-channel case), every one of them among the exempted.
"""
import ctypes as C
import functools
import glob
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import fengine_ref as ref
import guarded

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")


def _fused_ok(F, P):
    return 16 <= F <= 4096 and F & (F - 1) == 0 and P <= 16


def _routes(blk, F, P):
    """yields the route names after asserting them: the geometry's own route, then (where that was the fused one) the forced generic one"""
    if _fused_ok(F, P):
        assert blk.route().startswith("fused pow2 F=%d P=%d" % (F, P)), blk.route()
        yield blk.route()
        blk.set_generic(True)
    assert blk.route().startswith("generic F=%d P=%d" % (F, P)), blk.route()
    yield blk.route()
    blk.set_generic(False)


def _run(blk, xs, n, t0=0, in_off=0, out_off=0):
    """work_device for frames t0 .. t0 + n of the history-prefixed streams xs, on guard-banded buffers; offsets in items of the buffer's
    dtype past a 16-byte boundary.  Returns int8 [n][S][F][npol][2]."""
    import torch
    F, P = blk.num_channels, blk.taps_per_channel
    items = blk.items_per_input(n)
    ins = [guarded.guarded_input(np.asarray(x[t0 * F:t0 * F + items], np.complex64), guarded.pad_items(8, F), in_off, "cuda") for x in xs]
    wo, vo = guarded.guarded_output(n * blk.frame_bytes(), np.int8, guarded.pad_items(1, blk.frame_bytes()), out_off, "cuda")
    vo.fill_(-128)
    assert blk.work_device(n, [v for _, v in ins], [vo]) == n
    torch.cuda.synchronize()
    for w, v in ins:
        guarded.check_guards(w, v, "input")
    guarded.check_guards(wo, vo, "output", interior=False)
    y = guarded.to_numpy(vo)
    assert not (y == -128).any(), "an output byte was not written (or -128 was produced)"
    return y.reshape(n, blk.num_inputs, F, blk.npol, 2)


# ---- 1. exact pins -------------------------------------------------------------------------------------------------------------
# (S, npol, F, T): T is not a multiple of the 4096 / F frames of a group
PINS = [(3, 1, 16, 300), (2, 2, 64, 70), (1, 2, 4096, 3)]


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("S,npol,F,T", PINS)
def test_constants_land_in_channel_zero(gpu, pkg, S, npol, F, T, shift):
    """input r is the constant c_r, h = ones, P = 1, gain 1 / F: out[t][s][0][p] = c_r and every other channel exactly 0 (every sum of
    the transform is exact: small integers times a power of two, and differences of equal values)"""
    R = S * npol
    c = [complex(3 + r, -(2 + r)) for r in range(R)]
    xs = [np.full(T * F, v, np.complex64) for v in c]
    want = np.zeros((T, S, F, npol, 2), np.int8)
    for r, v in enumerate(c):
        want[:, r // npol, F // 2 if shift else 0, r % npol] = (v.real, v.imag)
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, None, 1, shift, np.full((R, F), 1.0 / F, np.float32))
    for route in _routes(blk, F, 1):
        assert np.array_equal(_run(blk, xs, T), want), route
    assert not blk.clips().any()


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("S,npol,F,T", PINS)
def test_tones_land_in_their_channels(gpu, pkg, S, npol, F, T, shift):
    """input r is a tone on bin k_r with amplitude 100.25 j^r after the gain 1 / F: (+-100, 0) or (0, +-100) in channel k_r, 0 elsewhere
    (leakage of the float32 samples and arithmetic stays below 0.01, and 100.25 is 0.25 from a boundary)"""
    R = S * npol
    n = np.arange(T * F)
    k = [(3 + 5 * r) % F for r in range(R)]
    xs = [(100.25 * 1j ** r * np.exp(2j * np.pi * k[r] * (n % F) / F)).astype(np.complex64) for r in range(R)]
    want = np.zeros((T, S, F, npol, 2), np.int8)
    for r in range(R):
        v = 100 * 1j ** r
        want[:, r // npol, (k[r] + F // 2) % F if shift else k[r], r % npol] = (int(v.real), int(v.imag))
    res = ref.fengine(xs, None, np.full((R, F), 1.0 / F), S, npol, F, 1, shift, T)
    assert np.array_equal(res.out, want)  # the yardstick agrees with the hand-made expectation
    off = np.abs(np.stack([res.v.real, res.v.imag], -1))[want == 0]
    assert off.max() < 0.01
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, None, 1, shift, np.full((R, F), 1.0 / F, np.float32))
    for route in _routes(blk, F, 1):
        assert np.array_equal(_run(blk, xs, T), want), route


# ---- 2. random data against the float64 reference -----------------------------------------------------------------------------
# (S, npol, F, P, T)
# (the last: more inputs than the 64 pointers one launch carries, so two launches, and two station batches on the generic route)
RANDOM = [(3, 1, 16, 1, 40), (2, 2, 64, 2, 9), (1, 2, 4096, 8, 3), (5, 2, 256, 4, 12), (2, 1, 1024, 16, 5), (2, 2, 48, 3, 20), (3, 1, 1000, 2, 4),
          (70, 1, 16, 2, 5)]


@functools.lru_cache(maxsize=None)
def _case(S, npol, F, P, T, rms=30.0, nans=0):
    """Gaussian streams, a windowed-sinc prototype, gains for `rms` per output component with a ripple over the channels; computed once"""
    rng = np.random.default_rng(100 + S * 7 + npol * 11 + F * 13 + P * 17 + T * 19 + int(rms))
    R = S * npol
    items = (T + P - 1) * F
    xs = [(rng.standard_normal(items) + 1j * rng.standard_normal(items)).astype(np.complex64) for _ in range(R)]
    h = ref.sinc_taps(F, P)
    X, _ = ref.spectra(xs, h, F, P, T)
    level = np.sqrt((np.abs(X) ** 2).mean(axis=(1, 2)) / 2)
    g = ((rms / level)[:, None] * (1.0 + 0.1 * np.cos(2 * np.pi * np.arange(F) / F + np.arange(R)[:, None]))).astype(np.float32)
    for i in range(nans):  # a NaN item poisons the P frames whose window holds it, every channel of them
        r = (i * 3 + 1) % R
        xs[r][(items // 2 + 37 * i) % items] = complex(np.nan, np.nan)
    res = ref.fengine(xs, h, g, S, npol, F, P, F % 2 == 0, T)
    for a in xs + [h, g, res.out, res.d, res.delta, res.clip]:
        a.setflags(write=False)
    return xs, h, g, res


def _compare(y, res, what):
    """decided components equal the reference; the others are a neighbour; returns (exempt share, components that differed)"""
    dec = res.decided()
    diff = y.astype(np.int16) - res.out.astype(np.int16)
    share, ndiff = 1.0 - dec.mean(), int((diff != 0).sum())
    print("%s: delta max %.2e, exempt share %.4f %%, components that differed %d of %d" % (what, res.delta.max(), 100 * share, ndiff, diff.size))
    assert not diff[dec].any(), what
    assert np.abs(diff).max() <= 1, what
    assert share <= 0.01, what
    return share, ndiff


@pytest.mark.parametrize("S,npol,F,P,T", RANDOM)
def test_random_against_float64(gpu, pkg, S, npol, F, P, T):
    xs, h, g, res = _case(S, npol, F, P, T)
    if F in (16, 256, 4096):
        assert res.delta.max() <= 2e-3  # the shapes at which a looser bound would exempt about 1 %
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, F % 2 == 0, g)
    assert np.array_equal(blk.gains(), g) and blk.frame_bytes() == 2 * S * F * npol and blk.history_items() == (P - 1) * F
    for route in _routes(blk, F, P):
        _compare(_run(blk, xs, T), res, "%s %s" % ((S, npol, F, P, T), route))


def test_generic_batches_of_frames(gpu, pkg):
    """F = 16384 is beyond the fused kernel; with 2 x 2 inputs the generic route's workspace holds 64 frames, so 66 frames are two batches
    (64 + 2): the reference's bits where float32 can decide, and the same bits as calls cut elsewhere"""
    S, npol, F, P, T = 2, 2, 16384, 1, 66
    xs, h, g, res = _case(S, npol, F, P, T)
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g)
    assert blk.route() == "generic F=16384 P=1 npol=2 batch=2x64"
    whole = _run(blk, xs, T)
    _compare(whole, res, "generic, two batches of frames")
    assert np.array_equal(np.concatenate([_run(blk, xs, 1), _run(blk, xs, 65, 1)]), whole)


# ---- 3. saturation and clips ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,npol,F,P,T,nans", [(2, 2, 64, 2, 70, 3), (1, 2, 1024, 4, 40, 1), (2, 2, 48, 3, 20, 1)])
def test_saturation_and_clip_counters(gpu, pkg, S, npol, F, P, T, nans):
    """gains for an rms of 77.5: a tenth of the components beyond +-127.5; a few NaN items (each makes P whole frames of its input NaN)"""
    xs, h, g, res = _case(S, npol, F, P, T, 77.5, nans)
    assert 0.05 < res.clip.mean() < 0.2 and np.isnan(res.v).any()
    dec = res.decided()
    lo, room = res.clips(dec), res.undecided_per_input()
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, F % 2 == 0, g)
    for route in _routes(blk, F, P):
        blk.clips(reset=True)
        y = _run(blk, xs, T)  # (_run asserts that no byte is -128)
        _compare(y, res, "saturating %s %s" % ((S, npol, F, P, T), route))
        nanq = np.isnan(np.stack([res.v.real, res.v.imag], -1))
        assert not y[nanq].any()  # a NaN component is 0
        got = blk.clips()
        assert np.all(got >= lo) and np.all(got <= lo + room.astype(np.uint64)), (route, got, lo, room)
        assert np.array_equal(blk.clips(reset=True), got) and not blk.clips().any()  # reset returns the totals, then zero
        totals = []
        for cuts in ((T,), (1, T // 2, T - 1 - T // 2), (T - 1, 1)):
            t0 = 0
            for n in cuts:
                _run(blk, xs, n, t0)
                t0 += n
            totals.append(blk.clips(reset=True))
        assert np.array_equal(totals[0], got) and np.array_equal(totals[1], got) and np.array_equal(totals[2], got), route


# ---- 4. split invariance and alignment ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,npol,F,P,T", [(3, 1, 16, 3, 300), (2, 2, 64, 2, 70), (1, 2, 4096, 8, 3), (2, 2, 48, 3, 20)])
def test_split_invariance_and_alignment(gpu, pkg, S, npol, F, P, T):
    xs, h, g, res = _case(S, npol, F, P, T)
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, F % 2 == 0, g)
    for route in _routes(blk, F, P):
        whole = _run(blk, xs, T)
        parts, t0 = [], 0
        for n in (1, T // 3, T - 1 - T // 3):
            parts.append(_run(blk, xs, n, t0))
            t0 += n
        assert np.array_equal(np.concatenate(parts), whole), route
        assert np.array_equal(_run(blk, xs, T, 0, 1, 0), whole), route   # inputs 8-byte but not 16-byte aligned
        assert np.array_equal(_run(blk, xs, T, 0, 0, 2), whole), route   # out 2-byte aligned
        assert np.array_equal(_run(blk, xs, T, 0, 1, 6), whole), route


# ---- 5. gain updates ------------------------------------------------------------------------------------------------------------
def test_set_gains_between_enqueued_calls(gpu, pkg):
    """two work_dev calls on one stream with set_gains between them and no synchronisation: old gains entirely, then new entirely"""
    import torch
    S, npol, F, P, T = 5, 2, 256, 4, 12
    xs, h, g, res = _case(S, npol, F, P, T)
    g2 = (g * 0.5).astype(np.float32)
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g)
    d_x = [torch.from_numpy(x).cuda() for x in xs]
    for route in _routes(blk, F, P):
        blk.set_gains(g)
        o1 = torch.full((T * blk.frame_bytes(),), -128, dtype=torch.int8, device="cuda")
        o2 = torch.full_like(o1, -128)
        want1 = _run(blk, xs, T)
        blk.set_gains(g2)
        want2 = _run(blk, xs, T)
        assert not np.array_equal(want1, want2)
        blk.set_gains(g)
        torch.cuda.synchronize()
        blk.work_device(T, d_x, [o1])
        blk.set_gains(g2)
        blk.work_device(T, d_x, [o2])
        torch.cuda.synchronize()
        assert np.array_equal(o1.cpu().numpy().reshape(want1.shape), want1), route
        assert np.array_equal(o2.cpu().numpy().reshape(want2.shape), want2), route
        assert np.array_equal(blk.gains(), g2)


def test_set_input_gain_changes_one_input(gpu, pkg):
    S, npol, F, P, T = 5, 2, 256, 4, 12
    xs, h, g, res = _case(S, npol, F, P, T)
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g)
    r = 7  # station 3, polarisation 1
    gr = (g[r] * 0.25).astype(np.float32)
    g2 = g.copy()
    g2[r] = gr
    res2 = ref.fengine(xs, h, g2, S, npol, F, P, True, T)
    for route in _routes(blk, F, P):
        blk.set_gains(g)
        before = _run(blk, xs, T)
        blk.set_input_gain(r, gr)
        assert np.array_equal(blk.gains(), g2)
        after = _run(blk, xs, T)
        _compare(after, res2, "one input's gain " + route)
        same = np.ones((S, npol), bool)
        same[r // npol, r % npol] = False
        assert np.array_equal(after.transpose(1, 3, 0, 2, 4)[same], before.transpose(1, 3, 0, 2, 4)[same]), route
        assert not np.array_equal(after[:, r // npol, :, r % npol], before[:, r // npol, :, r % npol])
    for bad in (-1, S * npol):
        with pytest.raises(pkg.Mi355Error):
            blk.set_input_gain(bad, gr)
    assert np.array_equal(blk.gains(), g2)  # a refused update changes nothing


# ---- 6. refusals, zero frames, host equivalence --------------------------------------------------------------------------------------
def test_misaligned_and_overlapping_buffers_are_refused(gpu, pkg):
    import torch
    S, npol, F, P = 2, 1, 16, 2
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, None, P)
    L, h = pkg.lib(), blk._h
    buf = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    p = buf.data_ptr()

    def call(n, i0, i1, out):
        ptrs = (C.c_void_p * 2)(i0, i1)
        return L.mi355_fengine_work_dev(h, n, ptrs, C.c_void_p(out) if out is not None else None, None)

    # one frame reads 2 * 16 * 8 = 256 bytes per input and writes 64 bytes
    assert call(1, p, p + 1024, p + 4096) == 0
    assert call(1, p + 4, p + 1024, p + 8192) == -1      # an input not 8-byte aligned
    assert call(1, p, p + 1024 + 4, p + 8192) == -1
    assert call(1, p, p + 1024, p + 8192 + 1) == -1      # out not 2-byte aligned
    assert call(1, p, p + 1024, p + 1024 + 248) == -1    # out overlaps the second input's last item
    assert call(1, p + 8192 + 56, p + 1024, p + 8192) == -1  # the first input starts inside out
    assert call(1, p, p + 1024, p + 1024 + 256) == 0     # adjacent is not overlapping
    assert call(1, None, p + 1024, p + 8192) == -1 and call(1, p, p + 1024, None) == -1
    assert call(-1, p, p + 1024, p + 8192) == -1
    assert call((1 << 40) // 128 + 1, p, p + 1024, p + 8192) == -3
    assert L.mi355_fengine_work_dev(h, 1, None, C.c_void_p(p), None) == -1
    torch.cuda.synchronize()
    view = buf.cpu().numpy()
    assert not view[8192:].any()  # the refused calls launched nothing
    # out-of-range parameters and shift with an odd length, on a live context
    for args in ((0, 2, 16, None, 1), (2, 4097, 16, None, 1), (1, 2, 1, None, 1), (1, 2, 16, None, 0), (1, 2, 16, None, 1025), (1, 2, 15, None, 1, True)):
        with pytest.raises(pkg.Mi355Error):
            pkg.clFEngine(*GPU_ARGS, *args)
    x = torch.zeros(2 * 16, dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):
        blk.work_device(1, [x, x[:-1]], [buf])           # a short input tensor
    with pytest.raises(ValueError):
        blk.work_device(1, [x, x], [buf[:63]])
    with pytest.raises(ValueError):
        blk.work_device(1, [x], [buf])


def test_zero_frames_is_a_no_op(gpu, pkg):
    import torch
    blk = pkg.clFEngine(*GPU_ARGS, 1, 2, 16)
    out = torch.full((256,), 7, dtype=torch.int8, device="cuda")
    assert pkg.lib().mi355_fengine_work_dev(blk._h, 0, None, C.c_void_p(out.data_ptr()), None) == 0
    assert pkg.lib().mi355_fengine_work(blk._h, 0, None, None) == 0
    assert blk.work_device(0, [], [out]) == 0 and blk.work(0, [], [out]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and not blk.clips().any()


@pytest.mark.parametrize("S,npol,F,P,T", [(5, 2, 256, 4, 12), (2, 2, 48, 3, 20)])
def test_host_work_equals_device_work(gpu, pkg, S, npol, F, P, T):
    xs, h, g, res = _case(S, npol, F, P, T)
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g)
    for route in _routes(blk, F, P):
        y = np.full(T * blk.frame_bytes(), -128, np.int8)
        assert blk.work(T, xs, [y]) == T
        assert np.array_equal(y.reshape(T, S, F, npol, 2), _run(blk, xs, T)), route
    with pytest.raises(ValueError):
        blk.work(T + 1, xs, [np.zeros((T + 1) * blk.frame_bytes(), np.int8)])


def test_host_work_in_two_pieces(gpu, pkg):
    """A piece of the host path is 64 MiB of input over all inputs.  2 stations of 2 polarisations, 16 channels, P = 4 and
    64 MiB / (8 * 16 * 4) + 3 frames: one full piece and one of three frames, which sends the three frames of history it shares with
    the first again.  The bytes and the clip counts of ONE work_device call on either route, and the float64 reference."""
    S, npol, F, P = 2, 2, 16, 4
    R = S * npol
    T = (64 << 20) // (8 * F * R) + 3
    rng = np.random.default_rng(4242)
    items = (T + P - 1) * F
    xs = [(rng.standard_normal(items) + 1j * rng.standard_normal(items)).astype(np.complex64) for _ in range(R)]
    h = ref.sinc_taps(F, P)
    # unit-variance components through the bank and the transform come out with variance sum h^2: 30 rms per output component, with
    # the ripple of _case, so that some components clip
    g = (30.0 / np.sqrt((h.astype(np.float64) ** 2).sum()) * (1.0 + 0.1 * np.cos(2 * np.pi * np.arange(F) / F + np.arange(R)[:, None]))).astype(np.float32)
    res = ref.fengine(xs, h, g, S, npol, F, P, True, T)
    dev, blk = (pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g) for _ in range(2))
    for _ in zip(_routes(dev, F, P), _routes(blk, F, P)):
        want = _run(dev, xs, T)
        y = np.full(T * blk.frame_bytes(), -128, np.int8)
        assert blk.work(T, xs, [y]) == T
        y = y.reshape(T, S, F, npol, 2)
        assert np.array_equal(y, want), blk.route()
        clips = blk.clips(reset=True)
        assert np.array_equal(clips, dev.clips(reset=True)) and clips.any(), blk.route()
        _compare(y, res, "two pieces, %s" % blk.route())


# ---- 7. the chain ---------------------------------------------------------------------------------------------------------------
def test_frames_feed_the_xengine_and_the_beamformer(gpu, pkg):
    """the device's own frames go to clXEngine (BYTE) and to clBeamformer (VOLTAGE) without leaving the device; both are compared with
    numpy integer sums over those same frames"""
    import torch
    import beamform_ref
    S, npol, F, P, T, B = 4, 2, 64, 4, 32, 3
    xs, h, g, res = _case(S, npol, F, P, T)
    fe = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g)
    assert fe.route().startswith("fused")
    d_x = [torch.from_numpy(x).cuda() for x in xs]
    frames = torch.full((T * fe.frame_bytes(),), -128, dtype=torch.int8, device="cuda")
    fe.work_device(T, d_x, [frames])
    xe = pkg.clXEngine(*GPU_ARGS, False, pkg.DTYPE_BYTE, npol, S, 1, 0, F, T, [])
    assert xe.input_bytes() == T * fe.frame_bytes()
    vis = torch.zeros(xe.get_output_buffer_size(), dtype=torch.complex64, device="cuda")
    xe.xcorrelate_device(frames, vis)
    rng = np.random.default_rng(8)
    w = beamform_ref.weights(rng, S, F, npol, B)
    bf = pkg.clBeamformer(*GPU_ARGS, beamform_ref.VOLTAGE, npol, S, F, B, 1, False, w)
    assert bf.frame_bytes() == fe.frame_bytes()
    beams = torch.zeros(T * B * F * npol, dtype=torch.complex64, device="cuda")
    bf.work_device(T, [frames], [beams])
    torch.cuda.synchronize()
    x = frames.cpu().numpy().reshape(T, S, F, npol, 2)
    _compare(x, res, "chain frames")
    # V[f][k][p1 npol + p2] = sum_t x_s1p1 conj(x_s2p2), k = s1 (s1 + 1) / 2 + s2, in int64; the BYTE path scales by (1 / 127)^2
    rows = x.transpose(0, 1, 3, 2, 4).reshape(T, S * npol, F, 2).astype(np.int64)
    I, Q = rows[..., 0], rows[..., 1]
    re = np.einsum("trf,tuf->fru", I, I) + np.einsum("trf,tuf->fru", Q, Q)
    im = np.einsum("trf,tuf->fru", Q, I) - np.einsum("trf,tuf->fru", I, Q)
    s1, s2 = np.tril_indices(S)
    vr = np.zeros((F, s1.size, npol * npol), np.int64)
    vi = np.zeros_like(vr)
    for p1 in range(npol):
        for p2 in range(npol):
            vr[:, :, p1 * npol + p2] = re[:, s1 * npol + p1, s2 * npol + p2]
            vi[:, :, p1 * npol + p2] = im[:, s1 * npol + p1, s2 * npol + p2]
    kd = 0.007874015748031496063
    want = ((vr.astype(np.float64) * kd * kd).astype(np.float32) + 1j * (vi.astype(np.float64) * kd * kd).astype(np.float32)).astype(np.complex64)
    assert np.array_equal(vis.cpu().numpy(), want.reshape(-1))
    assert np.array_equal(beams.cpu().numpy(), beamform_ref.voltage(x, w).reshape(-1))


# ---- 8. the C++ block through pybind, and the CLI row -----------------------------------------------------------------------------
def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu, pkg):
    """the C++ block as the scheduler calls it: R complex streams with (P - 1) F items of history in front, one frame per output item"""
    mod = _pybind()
    S, npol, F, P, T = 5, 2, 256, 4, 12
    xs, h, g, res = _case(S, npol, F, P, T)
    fe = mod.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g.reshape(-1))
    assert fe.decimation() == F and fe.history() == (P - 1) * F + 1 and fe.frame_bytes() == 2 * S * F * npol
    assert fe.route().startswith("fused pow2 F=256 P=4") and np.array_equal(fe.gains(), g.reshape(-1))
    y = np.full(T * fe.frame_bytes(), -128, np.int8)
    assert fe.work(T, list(xs), [y]) == T
    blk = pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, True, g)
    assert np.array_equal(y.reshape(T, S, F, npol, 2), _run(blk, xs, T))
    got, lo = fe.clips(False), res.clips(res.decided())  # (4.25 sigma: a handful of the 61440 components do clip)
    assert got.dtype == np.uint64 and np.all(got >= lo) and np.all(got <= lo + res.undecided_per_input().astype(np.uint64))
    assert np.array_equal(fe.clips(True), got) and not fe.clips().any()
    fe.set_generic(True)
    assert fe.route().startswith("generic")
    fe.set_input_gain(0, np.zeros(F, np.float32))
    assert fe.work(T, list(xs), [y]) == T
    assert not y.reshape(T, S, F, npol, 2)[:, 0, :, 0].any()
    with pytest.raises(ValueError):
        fe.set_gains(g.reshape(-1)[:-1])
    with pytest.raises(ValueError):
        mod.clFEngine(*GPU_ARGS, npol, S, 255, [], 1, True)  # shift with an odd length


def test_cli_row(gpu):
    """test-clenabled-mi355 --fengine-only prints the checksum of a small run on generated streams: sum_i (i % 7 + 1) out_i over the
    output bytes in memory order"""
    r = subprocess.run([CLI, "--fengine-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    S, npol, F, P, T = 3, 2, 64, 2, 70
    state, R = 12345, S * npol
    items = (T + P - 1) * F
    vals = np.empty(2 * R * items, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    vals = (vals - 256 * (vals > 127)).astype(np.float32).reshape(R, items, 2)
    xs = [(vals[r2, :, 0] + 1j * vals[r2, :, 1]).astype(np.complex64) for r2 in range(R)]
    h = np.array([(1 + (i % 5)) * 0.25 for i in range(P * F)], np.float32)
    g = np.full((R, F), 1.0 / 512, np.float32)
    res = ref.fengine(xs, h, g, S, npol, F, P, True, T)
    i = np.arange(res.out.size)
    base = int(((i % 7 + 1) * res.out.reshape(-1).astype(np.int64)).sum())
    slack = int(((i % 7 + 1) * (~res.decided()).reshape(-1)).sum())  # an undecided component may be a neighbour
    got = int(re.search(r"^clFEngine checksum (-?\d+)$", r.stdout, re.M).group(1))
    assert abs(got - base) <= slack, (got, base, slack, r.stdout)
    rows = [l for l in r.stdout.splitlines() if l.startswith("clFEngine (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout


def test_generic_route_one_handle_two_streams(gpu, pkg):
    """the generic route's workspace handed between two streams: 6 calls per stream in turn with nothing waited for in between, the
    first of 1 frame and the others of 3, so the workspace grows after it has been used.  Every output (filled with -128 first) is byte
    for byte what a second handle gives for the same frames on one stream."""
    import torch
    S, npol, F, P, T = RANDOM[0]  # the smallest shape that runs the generic route above
    xs, h, g, _ = _case(S, npol, F, P, T)
    blk, single = (pkg.clFEngine(*GPU_ARGS, npol, S, F, h, P, F % 2 == 0, g) for _ in range(2))
    for b in (blk, single):
        b.set_generic(True)
        assert b.route().startswith("generic F=%d P=%d" % (F, P)), b.route()
    # stream s works on frames 3 s .. 3 s + 2
    d_xs = [[torch.tensor(x[3 * s * F:], device="cuda") for x in xs] for s in range(2)]
    out = lambda n: torch.full((n * blk.frame_bytes(),), -128, dtype=torch.int8, device="cuda")  # noqa: E731
    refs = {}
    for s in range(2):
        for n in (1, 3):
            refs[s, n] = out(n)
            assert single.work_device(n, [d[:blk.items_per_input(n)] for d in d_xs[s]], [refs[s, n]]) == n
            torch.cuda.synchronize()
            assert not (refs[s, n] == -128).any()
    count = lambda k, s: 1 if (k, s) == (0, 0) else 3  # noqa: E731
    streams = [torch.cuda.Stream() for _ in range(2)]
    ys = [[out(count(k, s)) for k in range(6)] for s in range(2)]
    torch.cuda.synchronize()
    for k in range(6):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                blk.work_device(count(k, s), [d[:blk.items_per_input(count(k, s))] for d in d_xs[s]], [ys[s][k]])
    torch.cuda.synchronize()
    for s in range(2):
        for k in range(6):
            assert torch.equal(ys[s][k], refs[s, count(k, s)]), (s, k)
