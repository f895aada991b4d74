"""GPU: every route of the device-resident path stays inside the caller's buffers, at any alignment the C ABI accepts.

work_device() runs the kernels on the caller's own buffers.  Here every buffer is a view into a larger allocation (tests/guarded.py):
NaN around the inputs (a read outside that reaches an output shows, even through a zero tap or window value), a sentinel bit pattern
around the outputs (a store outside shows), NaN inside the outputs before the call (an item never written shows).  Every case runs
with the input and the output 0 and 1 item past a 16-byte boundary (8-byte aligned only for complex64), in all combinations the
contract allows; the interior is compared with the float64 reference and the tolerance the route's own test uses.  Where the
launcher does not look at the address the offset runs must equal the aligned run bit for bit.  Pads: max(64 KiB, one frame or block
of the operation), at most 1 MiB, on each side (guarded.pad_items).  The refusals of the pointer contract are at the end, the host
path's copy-back side (numpy outputs inside sentinel-filled arrays) before them.  DESIGN.md, 'Buffer contract', says the same in words.

This file covers clFFT, the filters, the channelizer, the math and elementwise blocks and the FFT correlator.  The X-engine (every label
of last_route(), several windows per call, the sharded engine, pack3d_device and the host calls) is in tests/test_xengine_bounds_gpu.py,
which imports the helpers below; the resampler, the synthesizer, the loops and clXCorrelate carry their guard tests in their own files.

Routes are forced with the switches the code has and named in the test ids.  Not reachable from this process: the segment loop of k_ols
for a partitioned filter (MI355_OLS_PART_ONE_PASS is read once per process), the one-wave clFFT geometry (MI355_FFT_WAVE_GEO, same).
Those run, without the guard bands, in child processes that start with the variable set: tests/test_switches_once_gpu.py.
"""
import numpy as np
import pytest
import torch

from conftest import GPU_ARGS, crandn, relerr
from fft_ref import fft_bound_check, fft_bound_kind, fft_frames64
from guarded import SENTINEL, GuardError, check_guards, guarded_input, guarded_output, pad_items, to_numpy
from test_fft_gpu import _np_fft_block
from test_fft_sched_gpu import _frames
from test_xcorr_gpu import _np_xcorr

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda"
ALL4 = ((0, 0), (0, 1), (1, 0), (1, 1))


def _bits(t):
    return (torch.view_as_real(t) if t.is_complex() else t).contiguous().view(torch.int32)


def _run_offsets(call, ins, outs, offsets, check, bitwise):
    """ins: [(numpy array, unit_items)], outs: [(n_items, dtype, unit_items)]; offsets: (input offset, output offset) pairs in items.
    call(in_views, out_views) enqueues the work; check([numpy outputs]) compares with the reference.  Guards after every run; with
    `bitwise` every run after the first must equal the first bit for bit (and only the first is compared with the reference)."""
    first = None
    for oi, oo in offsets:
        gi = [guarded_input(a, pad_items(a.dtype.itemsize, u), oi, DEV) for a, u in ins]
        go = [guarded_output(n, dt, pad_items(np.dtype(dt).itemsize, u), oo, DEV) for n, dt, u in outs]
        for (_, v), o in [(g, oi) for g in gi] + [(g, oo) for g in go]:
            assert v.data_ptr() % 16 == (o * v.element_size()) % 16
        call([v for _, v in gi], [v for _, v in go])
        torch.cuda.synchronize()
        for k, (w, v) in enumerate(gi):
            check_guards(w, v, "input %d at offset %d" % (k, oi))
        for k, (w, v) in enumerate(go):
            check_guards(w, v, "output %d at offsets in %d / out %d" % (k, oi, oo))
        if first is None or not bitwise:
            check([to_numpy(v) for _, v in go])
        if bitwise:
            if first is None:
                first = [v.clone() for _, v in go]
            else:
                for k, (a, (_, v)) in enumerate(zip(first, go)):
                    assert torch.equal(_bits(a), _bits(v)), "output %d at offsets in %d / out %d differs from the aligned run" % (k, oi, oo)


@pytest.mark.parametrize("dtype", [np.complex64, np.float32, np.int32], ids=lambda d: np.dtype(d).name)
def test_guards_catch_the_stand_ins_on_device_tensors(gpu, dtype):
    """the stand-ins of tests/test_guarded.py (plain torch operations that stray by one item INSIDE their own allocation: nothing faults)
    on device tensors: the checks used below see on the device what they see on the CPU"""
    import test_guarded as tg
    for oi, oo in ALL4:
        got, ref = tg._run(tg._correct, dtype, oi, oo, h=1, device=DEV)
        assert np.array_equal(got, ref)
        for standin, where, index in ((tg._writes_one_after, "after", tg.N), (tg._writes_one_before, "before", -1),
                                      (tg._leaves_last_unwritten, "interior", tg.N - 1)) + \
                                     (((tg._reads_one_past_input, "interior", tg.N - 1),) if dtype != np.int32 else ()):
            with pytest.raises(GuardError) as e:
                tg._run(standin, dtype, oi, oo, device=DEV)
            assert (e.value.where, e.value.index) == (where, index), standin.__name__


def _setenv(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ---------------------------------------------------------------------------------------------------------------- clFFT

MODES = {"fwd_shift_win": (True, True, True, False), "bwd_shift": (False, True, False, False), "fwd": (True, False, False, False),
         "bwd_win": (False, False, True, False), "real_fwd_shift_win": (True, True, True, True), "bwd": (False, False, False, False)}
SMALL = ["fwd_shift_win", "bwd_shift", "fwd", "bwd_win", "real_fwd_shift_win"]
BIG = ["fwd_shift_win", "bwd"]  # the persistent-sized calls (128 MiB each way): both directions, the shift on and off
FFT_CASES = []


def _fft_add(route, n, frames, modes, env=None):
    tag = "".join("-%s=%s" % (k.replace("MI355_FFT_", ""), v) for k, v in (env or {}).items())
    for fr in frames:
        for m in modes:
            FFT_CASES.append(pytest.param(route, n, fr, m, env or {}, id="%s%s-n%d-frames_%s-%s" % (route, tag, n, fr, m)))


for _n in (2, 8, 64):
    _g = 4096 // _n
    _fft_add("one_pass_lds_redistributed", _n, (1, 3 * _g - 1, 3 * _g + 1), SMALL)
for _n in (256, 1024, 4096):
    _g = 4096 // _n
    _fft_add("one_pass_grid_stride", _n, (1, 3 * _g - 1, 3 * _g + 1), SMALL)
for _n in (1024, 4096):  # (the per-call switches innermost: consecutive cases share input and reference, 128 MiB each)
    for _fr in ("persistent+0", "persistent+37"):
        for _m in BIG + (["real_fwd_shift_win"] if _fr == "persistent+37" else []):
            for _s in ("0", "1"):
                _fft_add("persistent_prefetch", _n, (_fr,), [_m], {"MI355_FFT_SCHED": _s})
            if _n == 4096 and _fr == "persistent+37" and _m in BIG:
                for _p in ("0", "2"):
                    _fft_add("persistent_sized", 4096, (_fr,), [_m], {"MI355_FFT_PREFETCH": _p})
for _n in (8192, 16384, 32768):
    _fft_add("sub_transform_kernel", _n, (1, 3, 5), SMALL)
for _n in (65536, 131072, 1048576):
    _fft_add("two_tile_passes", _n, (1, 3), SMALL)
_fft_add("four_passes", 1 << 21, (1,), SMALL)
for _n in (12, 48, 100, 675, 1000, 3584, 3840, 7680, 13312, 15360):
    _fft_add("mixed_radix_one_pass", _n, (1, 11), SMALL)
for _v in ("0", "1"):
    _fft_add("mixed_radix_one_pass", 96, (1, 11), SMALL, {"MI355_FFT_MR_VARIANT": _v})
_fft_add("mixed_radix_one_pass_grid_stride", 1000, (20011,), ["fwd"])
for _n, _f in ((16000, (1, 3)), (22050, (1, 2)), (50625, (1, 2)), (921600, (1, 2))):
    _fft_add("mixed_radix_two_passes", _n, _f, SMALL)
for _n in (4099, 8191):
    _fft_add("chirpz_fused", _n, (1, 7), SMALL)
_fft_add("chirpz_fused", 1200, (1, 7), SMALL, {"MI355_FFT_NO_MR": "1"})
# (16385 points: m = 65536, the two tile passes inside; 16383 is the length whose m is 32768; 100003: m = 262144)
for _n in (16383, 16385, 100003):
    _fft_add("chirpz_unfused", _n, (1, 2), SMALL)

_PLAN = {"one_pass_lds_redistributed": "one pass", "one_pass_grid_stride": "one pass", "persistent_prefetch": "one pass", "persistent_sized": "one pass",
         "sub_transform_kernel": "one pass", "two_tile_passes": "two tile passes", "four_passes": "four passes",
         "mixed_radix_one_pass": "mixed radix ", "mixed_radix_one_pass_grid_stride": "mixed radix ", "mixed_radix_two_passes": "mixed radix, two passes",
         "chirpz_fused": "chirp-z", "chirpz_unfused": "chirp-z"}


def _plan_text(gpu, n):
    import ctypes
    b = ctypes.create_string_buffer(200)
    assert gpu.lib().mi355_fft_plan_text(n, b, 200) == 0
    return b.value.decode()


def _fft_ref(oracle, n, fwd, w, shift, x, real):
    if n & (n - 1) == 0 or n <= 2401:
        return oracle.fft_block(n, fwd, w, shift, oracle.DTYPE_FLOAT if real else oracle.DTYPE_COMPLEX, x, f64=True)
    return _np_fft_block(n, fwd, w, shift, x.astype(np.complex64))


_REF_CACHE = {}


def _fft_data(oracle, n, frames, mode, sampled):
    """input, window, reference and unrounded float64 reference (fft_ref.fft_frames64, for the per-frame bounds) of a case; kept for the
    next case when only a per-call switch differs (the persistent-sized calls are 128 MiB each way)"""
    key = (n, frames, mode)
    if key not in _REF_CACHE:
        _REF_CACHE.clear()
        fwd, shift, win, real = MODES[mode]
        rng = np.random.default_rng(n * 31 + frames)
        x = rng.standard_normal(frames * n).astype(np.float32) if real else crandn(rng, frames * n)
        w = oracle.window(oracle.WIN_BLACKMAN_HARRIS, n) if win else None
        if sampled:  # (the oracle's DFT of a length that is not a power of two is O(n^2): first, middle and last frames, as the route's own test does)
            ref = {f0: _fft_ref(oracle, n, fwd, w, shift, x[f0 * n:(f0 + 3) * n], real) for f0 in (0, frames // 2, frames - 3)}
            ref64 = {f0: fft_frames64(n, fwd, w, shift, x[f0 * n:(f0 + 3) * n], real) for f0 in ref}
        else:
            ref = _fft_ref(oracle, n, fwd, w, shift, x, real)
            ref64 = fft_frames64(n, fwd, w, shift, x, real)
        _REF_CACHE[key] = (x, w, ref, ref64)
    return _REF_CACHE[key]


@pytest.mark.parametrize("route,n,frames,mode,env", FFT_CASES)
def test_clfft_stays_inside_its_buffers(gpu, oracle, monkeypatch, route, n, frames, mode, env):
    fwd, shift, win, real = MODES[mode]
    if isinstance(frames, str):
        frames = _frames(n, int(frames.split("+")[1]))
        assert (frames + max(4096 // n, 1) - 1) // max(4096 // n, 1) >= torch.cuda.get_device_properties(0).multi_processor_count * 16
    chirpz = route.startswith("chirpz")
    if not env.get("MI355_FFT_NO_MR"):
        assert _plan_text(gpu, n).startswith(_PLAN[route]), _plan_text(gpu, n)
    if route == "chirpz_fused":
        assert 2 * n - 1 <= 16384
    _setenv(monkeypatch, env)
    x, w, ref, ref64 = _fft_data(oracle, n, frames, mode, sampled=frames > 10000 and n == 1000)
    blk = gpu.clFFT(n, gpu.CLFFT_FORWARD if fwd else gpu.CLFFT_BACKWARD, [] if w is None else w, gpu.DTYPE_FLOAT if real else gpu.DTYPE_COMPLEX,
                    *GPU_ARGS, 0, 1, shift)
    # the input of a length above 4096 that is not a chirp-z length must be 16-byte aligned (its refusal: test_refusals); a float
    # input moves by two items, the smallest step the 8-byte rule allows
    step = 2 if real else 1
    offsets = [(oi * step, oo) for oi, oo in ALL4 if oi == 0 or chirpz or n <= 4096]

    def check(outs):
        kind = fft_bound_kind(blk.last_route())  # every frame inside the per-bin and per-frame bounds of the route that ran
        if isinstance(ref, dict):
            for f0, r in ref.items():
                assert relerr(outs[0][f0 * n:(f0 + 3) * n], r) <= TOL, f0
                fft_bound_check(outs[0][f0 * n:(f0 + 3) * n], ref64[f0], n, kind, what=blk.last_route())
        else:
            err = relerr(outs[0], ref)
            print("relerr %.3g" % err)
            assert err <= TOL
            print("bounds used %.3f (bin) %.3f (rss)" % fft_bound_check(outs[0], ref64, n, kind, what=blk.last_route()))

    _run_offsets(lambda i, o: blk.work_device(frames, i, o), [(x, n)], [(frames * n, np.complex64, n)], offsets, check,
                 bitwise=route.startswith(("one_pass", "persistent", "mixed_radix_one_pass")))


# ------------------------------------------------------------------------------------------- clFilter / clComplexFilter

def _pick_nf(ntaps):
    """pick_fft_size() of filter.hip (the test asserts fftsize() agrees)"""
    nf = 2
    while nf < 2 * ntaps:
        nf <<= 1
    nf = max(nf, 256)
    rate = lambda n: 413.0 if n <= 256 else 314.0 if n == 512 else 295.0 if n == 1024 else 292.0 if n == 2048 else 290.0  # noqa: E731
    s0 = (ntaps - 1 + 15) & ~15
    best, best_score, c = nf, 0.0, nf
    while c <= 4096 and c <= 8 * nf:
        score = rate(c) * ((c - s0) & ~15) / c
        if score > best_score * 1.02:
            best_score, best = score, c
        c <<= 1
    return best


def _ols_tile(ntaps, nf, wave):
    """undecimated outputs of one workgroup iteration of k_ols (launch_ols_g): block length L times the frames per iteration"""
    s0 = (ntaps - 1 + 15) & ~15
    L = nf - s0
    if L > 16:
        L &= ~15
    return L * ((1024 if wave else 4096) // nf)


FILTER_CASES = []


def _filt_add(route, ntaps, decim, ctaps, use_time, env, tile_y, in_offs=(0, 1), bitwise=False, nf=0, more=()):
    tag = "".join("-%s=%s" % (k.replace("MI355_", ""), v) for k, v in env.items())
    FILTER_CASES.append(pytest.param(ntaps, decim, ctaps, use_time, env, tile_y, in_offs, bitwise, nf, more,
                                     id="%s%s-%dtaps_%s-decim%d" % (route, tag, ntaps, "complex" if ctaps else "real", decim)))


for _nt, _force in ((3, 64), (3, 0), (30, 64), (30, 128), (65, 0), (65, 512), (300, 1024), (300, 2048), (300, 0), (1000, 2048), (1000, 0), (2048, 0)):
    _nf = _force or _pick_nf(_nt)
    for _geo in (("0", "1") if _nf <= 1024 else (None,)):
        _env = dict({"MI355_FILTER_FFT": str(_force)} if _force else {}, **({"MI355_FILTER_WAVE_GEO": _geo} if _geo else {}))
        for _d, _ct in ((1, False), (1, True), (2, False), (2, True), (3, False), (3, True)):
            _filt_add("k_ols_NF%d" % _nf, _nt, _d, _ct, False, _env, _ols_tile(_nt, _nf, _geo == "1"), bitwise=True, nf=_nf)
for _nt in (2049, 5000):
    for _env in ({}, {"MI355_OLS_UPS_WGS": "2"}, {"MI355_OLS_UPS_WGS": "1000"}):
        for _d, _ct in ((1, False), (3, False), (1, True), (2, True)):
            # 13-14 blocks of 2048 with a ragged end: MI355_OLS_UPS_WGS=2 walks runs of seven blocks, the last run shorter; and once 700 blocks,
            # where 1000 workgroups (one block each) differ from the default's runs of several blocks on up to 256 compute units
            _more = (2048 * 13 // _d + 77,) + ((2048 * 700 - 5,) if (_nt, _d, _ct) == (2049, 1, False) else ())
            _filt_add("k_ols_ups", _nt, _d, _ct, False, _env, 2048, bitwise=True, nf=4096, more=_more)
for _nt, _env in ((2049, {"MI355_OLS_UPS": "0"}), (5000, {"MI355_OLS_UPS": "0"}), (10241, {})):
    _seg = -(-_nt // -(-_nt // 2048))
    for _d, _ct in ((1, False), (3, False), (1, True), (2, True)):
        _filt_add("k_ols_part", _nt, _d, _ct, False, _env, (4096 - ((_seg - 1 + 15) & ~15)) & ~15, bitwise=True, nf=4096)
for _ct in (False, True):
    for _d in (1, 4):
        _filt_add("k_fir_td", 9, _d, _ct, True, {}, 2048)
    _filt_add("k_fir_mfma", 65, 1, _ct, True, {}, 4096)
    _filt_add("k_fir_mfma_dec", 129, 2, _ct, True, {}, 4096)
    _filt_add("k_fir_mfma_dec", 65, 16, _ct, True, {"MI355_FIR_DEC_KERNEL": "all"}, 4096)
    # 65 taps, KP = 72: k_fir_dec2 tiles of (3072 - 72) / 16 + 1 = 188 outputs, and 256 (a whole round of threads) at decimation 9;
    # k_fir_dec_lds tiles of (8192 - 65) / D + 1 outputs
    _filt_add("k_fir_dec2_even", 65, 16, _ct, True, {"MI355_FIR_DEC_KERNEL": "lds"}, 188 * 16, in_offs=(0,))
    _filt_add("k_fir_dec2_odd", 65, 9, _ct, True, {"MI355_FIR_DEC_KERNEL": "lds"}, 256 * 9, in_offs=(0,))
    for _d in (16, 9):
        _filt_add("k_fir_dec_lds_input_8_byte_aligned", 65, _d, _ct, True, {"MI355_FIR_DEC_KERNEL": "lds"}, ((8192 - 65) // _d + 1) * _d, in_offs=(1,))
        _filt_add("k_fir_dec_lds", 65, _d, _ct, True, {"MI355_FIR_DEC_KERNEL": "lds", "MI355_FIR_DEC2_OFF": "1"}, ((8192 - 65) // _d + 1) * _d, in_offs=(0,))
    _filt_add("k_fir_td_dec", 77, 700, _ct, True, {}, 256 * 700)
    _filt_add("k_fir_td_dec", 65, 40, _ct, True, {"MI355_FIR_DEC_KERNEL": "per_output"}, 256 * 40)


@pytest.mark.parametrize("ntaps,decim,ctaps,use_time,env,tile_y,in_offs,bitwise,nf,more", FILTER_CASES)
def test_filter_stays_inside_its_buffers(gpu, oracle, monkeypatch, ntaps, decim, ctaps, use_time, env, tile_y, in_offs, bitwise, nf, more):
    """The input view is exactly nout * decim + ntaps - 1 items; nout = 1, one tile of the kernel less one and plus one output, several
    tiles with a ragged end (tile_y: undecimated outputs of one workgroup iteration, read off launch_filter / launch_ols_g), and `more`.
    Which kernel a time-domain case runs follows from launch_filter's choice (its rate model and the switches in the id); the library
    has no query for it, so the ids and tile lengths here have to be re-read against launch_filter when a constant of that model moves."""
    _setenv(monkeypatch, env)
    rng = np.random.default_rng(ntaps * 13 + decim)
    if ctaps:
        taps = (crandn(rng, ntaps) / np.sqrt(ntaps)).astype(np.complex64)
        blk = gpu.clComplexFilter(*GPU_ARGS, decim, taps, 1, 0, use_time=use_time)
    else:
        taps = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        blk = gpu.clFilter(*GPU_ARGS, decim, taps, 1, 0, use_time)
    assert blk.fftsize() == nf
    tile = max(tile_y // decim, 2)
    offsets = [(oi, oo) for oi in in_offs for oo in (0, 1)]
    for nout in sorted({1, tile - 1, tile + 1, 3 * tile + tile // 3 + 1} | set(more)):
        xh = crandn(rng, nout * decim + ntaps - 1)
        ref = (oracle.fir_ccc if ctaps else oracle.fir_ccf)(taps, xh, nout, decim)

        def check(outs):
            err = relerr(outs[0], ref)
            print("nout %d relerr %.3g" % (nout, err))
            assert err <= TOL, nout

        _run_offsets(lambda i, o: blk.work_device(nout, i, o), [(xh, tile * decim + ntaps)], [(nout, np.complex64, tile)], offsets, check, bitwise)


# --------------------------------------------------------------------------------------------- clPolyphaseChannelizer

PFB_CASES = []


def _pfb_add(route, M, R, per_arm, nmap, steps, env=None, nbuf=1):
    tag = "".join("-%s" % k.replace("MI355_PFB_", "") for k in (env or {}))
    PFB_CASES.append(pytest.param(M, R, per_arm, nmap, steps, env or {}, nbuf,
                                  id="%s%s-%dch_R%d-%dtaps_per_arm-map%d%s" % (route, tag, M, R, per_arm, nmap, "-nbuf%d" % nbuf if nbuf > 1 else "")))


for _M in (64, 2, 16, 256):
    _pfb_add("fast_path", _M, _M, 32, _M, 4096 // _M + 37)
_pfb_add("fast_path", 64, 64, 32, 64, 101, nbuf=3)
_pfb_add("fast_path_partial_map", 64, 64, 32, 5, 101)
for _M, _pa, _st in ((1024, 32, 45), (1000, 7, 83), (7, 5, 3000)):
    _pfb_add("two_kernels", _M, _M, _pa, _M, _st)
    _pfb_add("two_kernels", _M, _M, _pa, _M, _st, {"MI355_PFB_NO_FIR_RING": "1"})
_pfb_add("two_kernels", 1000, 1000, 7, 999, 83)
_pfb_add("two_kernels", 1024, 1024, 32, 1024, 45, nbuf=3)
for _M, _R, _pa, _st in ((64, 32, 8, 203), (128, 32, 32, 134)):
    _pfb_add("oversampled_ring", _M, _R, _pa, _M, _st)
    _pfb_add("oversampled", _M, _R, _pa, _M, _st, {"MI355_PFB_NO_FAST_OVERSAMPLED": "1"})
_pfb_add("oversampled_ring_partial_map", 128, 32, 32, 50, 134)
_pfb_add("oversampled_ring", 64, 32, 8, 64, 204, nbuf=3)
_pfb_add("filters_and_transform_in_one_kernel", 100, 100, 32, 100, 70)
_pfb_add("filters_and_transform_in_one_kernel", 100, 100, 32, 100, 70, nbuf=3)
_pfb_add("two_kernels_mixed_radix", 100, 100, 32, 100, 70, {"MI355_PFB_NO_MR_FUSED": "1"})
# (a partial map does not keep k_pfb_mr away: it writes a scratch that k_pfb_map gathers from)
_pfb_add("filters_and_transform_in_one_kernel_partial_map", 100, 100, 32, 37, 70)
_pfb_add("two_kernels_mixed_radix_partial_map", 100, 100, 32, 37, 70, {"MI355_PFB_NO_MR_FUSED": "1"})
# ninputs_per_iter that does not divide the channel count, or not into 1, 2 or 4: the branch filters one output per thread (k_pfb_branches)
_pfb_add("generic_any_ratio", 100, 30, 5, 100, 83)
_pfb_add("generic_any_ratio", 12, 8, 7, 5, 84)
_pfb_add("generic_any_ratio", 3, 2, 48, 3, 300, nbuf=3)


@pytest.mark.parametrize("M,R,per_arm,nmap,steps,env,nbuf", PFB_CASES)
def test_channelizer_stays_inside_its_buffers(gpu, oracle, monkeypatch, M, R, per_arm, nmap, steps, env, nbuf):
    _setenv(monkeypatch, env)
    rng = np.random.default_rng(M * 17 + R + per_arm + nmap)
    K = M * per_arm - (M // 3 if per_arm % 2 and per_arm > 1 else 0)  # ragged last arm for the odd tap counts
    taps = (rng.standard_normal(K) / np.sqrt(per_arm)).astype(np.float32)
    buf = steps * R
    while buf % M:
        steps += 1
        buf = steps * R
    chmap = list(range(M)) if nmap == M else rng.permutation(M)[:nmap].tolist()
    blk = gpu.clPolyphaseChannelizer(*GPU_ARGS, taps, buf, M, R, chmap)
    nin, nout = blk.ninput() + (nbuf - 1) * buf, nbuf * blk.noutput()
    assert blk.ninput() == buf - R + K and blk.noutput() == nmap * buf // R
    xh = crandn(rng, nin)
    ref = np.concatenate([oracle.pfb(taps, buf, M, R, chmap, xh[b * buf:b * buf + blk.ninput()], f64=True) for b in range(nbuf)])

    def check(outs):
        err = relerr(outs[0], ref)
        print("relerr %.3g" % err)
        assert err <= TOL

    _run_offsets(lambda i, o: blk.work_device(i, o, nbuf=nbuf), [(xh, K)], [(nout, np.complex64, max(M, nmap))], ALL4, check, bitwise=True)


# ------------------------------------------------------------ clMathOp / clMathConst / elementwise / clxcorrelate_fft_vcf

SIZES = (1, 3, 4, 5, 8191, 8193, 100003)
_NP = {"COMPLEX": np.complex64, "FLOAT": np.float32, "INT": np.int32}


def _rand(rng, dt, n):
    if dt == "COMPLEX":
        return crandn(rng, n)
    if dt == "FLOAT":
        return rng.standard_normal(n).astype(np.float32)
    return rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("dt,op", [("COMPLEX", o) for o in ("MULTIPLY", "ADD", "SUBTRACT", "MULTIPLY_CONJUGATE")] +
                         [(d, o) for d in ("FLOAT", "INT") for o in ("MULTIPLY", "ADD", "SUBTRACT")])
def test_mathop_stays_inside_its_buffers(gpu, oracle, dt, op):
    """(16-byte aligned buffers only: the block's contract, see test_refusals)"""
    blk = gpu.clMathOp(getattr(gpu, "DTYPE_" + dt), *GPU_ARGS, getattr(gpu, "MATHOP_" + op))
    for n in SIZES:
        rng = np.random.default_rng(n)
        a, b = _rand(rng, dt, n), _rand(rng, dt, n)
        ref = oracle.mathop(getattr(oracle, "DTYPE_" + dt), getattr(oracle, "OP_" + op), a, b)

        def check(outs):
            if dt == "COMPLEX" and op.startswith("MULTIPLY"):
                assert relerr(outs[0], ref) <= TOL, n
            else:
                assert np.array_equal(outs[0], ref), n

        _run_offsets(lambda i, o: blk.work_device(n, i, o), [(a, 0), (b, 0)], [(n, _NP[dt], 0)], [(0, 0)], check, False)


@pytest.mark.parametrize("dt,op", [("COMPLEX", o) for o in ("MULTIPLY", "ADD", "SUBTRACT", "COMPLEX_CONJUGATE", "EMPTY_W_COPY")] +
                         [(d, o) for d in ("FLOAT", "INT") for o in ("MULTIPLY", "ADD", "SUBTRACT")])
def test_mathconst_stays_inside_its_buffers(gpu, oracle, dt, op):
    k = 7.0 if dt == "INT" else 2.5
    blk = gpu.clMathConst(getattr(gpu, "DTYPE_" + dt), *GPU_ARGS, k, getattr(gpu, "MATHOP_" + op))
    oop = {"COMPLEX_CONJUGATE": "CONJUGATE"}.get(op, op)
    for n in SIZES:
        a = _rand(np.random.default_rng(n + 1), dt, n)
        ref = oracle.mathconst(getattr(oracle, "DTYPE_" + dt), getattr(oracle, "OP_" + oop), k, a)

        def check(outs):
            assert np.array_equal(outs[0], ref), n

        _run_offsets(lambda i, o: blk.work_device(n, i, o), [(a, 0)], [(n, _NP[dt], 0)], [(0, 0)], check, False)


ELEM = {"clLog": 1, "clSNR": 2, "clComplexToMag": 3, "clComplexToArg": 4, "clComplexToMagPhase": 5, "clMagPhaseToComplex": 6, "clQuadratureDemod": 7}


@pytest.mark.parametrize("name", list(ELEM))
def test_elementwise_stays_inside_its_buffers(gpu, oracle, name):
    """every kind, both outputs of clComplexToMagPhase, the history item of clQuadratureDemod (its input is n + 1 items); any alignment
    of the item type is accepted (16-byte accesses when all pointers allow them, one item per thread otherwise)"""
    kind = ELEM[name]
    p0, p1 = {1: (2.5, -3.0), 2: (10.0, 1.0), 7: (0.75, 0.0)}.get(kind, (0.0, 0.0))
    blk = getattr(gpu, name)(*((p0,) + GPU_ARGS if kind == 7 else GPU_ARGS + ((p0, p1) if kind in (1, 2) else ())))
    for n in SIZES:
        rng = np.random.default_rng(n + kind)
        pos = lambda: (np.abs(rng.standard_normal(n)) + 0.05).astype(np.float32)  # noqa: E731
        ins = {1: lambda: [pos()], 2: lambda: [pos(), pos()], 6: lambda: [pos(), rng.uniform(-10, 10, n).astype(np.float32)],
               7: lambda: [crandn(rng, n + 1)]}.get(kind, lambda: [crandn(rng, n)])()
        refs = oracle.elem(kind, n, ins, p0, p1)
        odt = [np.complex64] if kind == 6 else [np.float32] * len(refs)

        def check(outs):
            for o, r in zip(outs, refs):
                assert relerr(o, r) <= TOL, (name, n)

        _run_offsets(lambda i, o: blk.work_device(n, i, o), [(a, 0) for a in ins], [(n, d, 0) for d in odt], ALL4, check, False)


@pytest.mark.parametrize("n,itype,nframes", [(256, 1, 37), (256, 2, 37), (1000, 2, 7)],
                         ids=["fused_kernel-spectra-256", "fused_kernel-time_series-256", "clfft_transforms-time_series-1000"])
def test_xcorr_fft_stays_inside_its_buffers(gpu, oracle, n, itype, nframes):
    ocl, sel, plat, dev = GPU_ARGS
    blk = gpu.clxcorrelate_fft_vcf(n, 3, ocl, sel, plat, dev, itype)
    rng = np.random.default_rng(n + itype)
    ins = [crandn(rng, nframes * n) for _ in range(3)]
    refs = oracle.xcorr_fft(n, itype, ins, use_f64=True) if n == 256 else _np_xcorr(n, itype, ins)

    def check(outs):
        for o, r in zip(outs, refs):
            assert relerr(o, r) <= TOL

    _run_offsets(lambda i, o: blk.work_device(nframes, i, o), [(a, n) for a in ins], [(nframes * n, np.float32, n)] * 2, ALL4, check, False)


# ------------------------------------------------------------------------------------------------ host path: the copy-back side

def _host_out(n, dtype, lead=3):
    """a numpy output of n items as a view `lead` items into a larger sentinel-filled array"""
    isz = np.dtype(dtype).itemsize
    pad = pad_items(isz)
    whole = np.full((2 * pad + n) * isz // 4, SENTINEL, np.int32).view(dtype)
    return whole, whole[pad + lead:pad + lead + n], pad + lead


def _host_check(whole, lo, n):
    w = whole.view(np.int32)
    k = whole.dtype.itemsize // 4
    assert np.all(w[:lo * k] == SENTINEL) and np.all(w[(lo + n) * k:] == SENTINEL), "the copy back wrote outside the output array"


DIRECT = 512 << 10  # kDirectBytes (common.h): a call whose largest buffer is at most this runs its kernels on the pinned staging itself
# (block, path, items).  Which paths a block's work() has differs, and the ids say which one a case takes:
#   clMathOp / clMathConst / clFFT / clFilter: the direct path, and the pipeline of staging chunks (total / 6 bytes each, 1 ... 8 MiB)
#     over HostPipe's four slots: 3.3 MiB = four chunks of 1 MiB, every slot used once; 5.5 MiB = six chunks, slots 0 and 1 used twice
#     (the wait for a slot's event and the delivery of its previous result beside the next input).  The filter sizes both by its
#     INPUT, decim x the output.
#   clPolyphaseChannelizer, elementwise: the direct path, else ONE staged transfer per call whatever its size (no chunks).
#   clxcorrelate_fft_vcf: no direct path; staged chunks of 64 MiB of input (all inputs together), so one chunk or, above that, two.
CHUNKS = {"four_chunks": 4, "six_chunks": 6}  # of 1 MiB: the call's sizing bytes lie in (chunks - 1, chunks] MiB
HOST_CASES = [("clMathOp", "direct", DIRECT // 8), ("clMathOp", "four_chunks", (3400 << 10) // 8 - 77),
              ("clMathOp", "six_chunks", (5600 << 10) // 8 - 77),
              ("clMathConst", "direct", DIRECT // 8), ("clMathConst", "four_chunks", (3400 << 10) // 8 - 77),
              ("clMathConst", "six_chunks", (5600 << 10) // 8 - 77),
              ("clFFT", "direct", DIRECT // 8), ("clFFT", "four_chunks", (3400 << 10) // 8 - 77),
              ("clFFT", "six_chunks", (5600 << 10) // 8 - 77),
              ("clFilter", "direct", 32700), ("clFilter", "four_chunks", (3400 << 10) // 16 - 77),
              ("clFilter", "six_chunks", (5600 << 10) // 16 - 77),
              ("clPolyphaseChannelizer", "direct", 64 * 900), ("clPolyphaseChannelizer", "one_staged_transfer", 64 * 6800),
              ("clComplexToMagPhase", "direct", 60001), ("clComplexToMagPhase", "one_staged_transfer", 435123),
              ("clxcorrelate_fft_vcf", "one_staged_chunk", 256 * 100), ("clxcorrelate_fft_vcf", "two_staged_chunks", 256 * 11000)]


@pytest.mark.parametrize("block,path,items", HOST_CASES, ids=["%s-%s" % c[:2] for c in HOST_CASES])
def test_host_path_copy_back_stays_inside_the_output(gpu, oracle, block, path, items):
    """work() on numpy buffers: the outputs are views into larger sentinel-filled arrays; the copy back (out of pinned staging after the
    direct path's wait, or slot by slot out of the pipeline) writes the output items and nothing else.  The sizes are checked here
    against the conditions the C side tests, so that an id does not name a path the call did not take."""
    rng = np.random.default_rng(len(block))
    direct = path == "direct"
    if block in ("clMathOp", "clMathConst", "clFFT"):
        assert (items * 8 <= DIRECT) == direct and (direct or items * 8 // 6 <= 1 << 20 < items * 8 // 3)
        sized = items // 1024 * 1024 * 8 if block == "clFFT" else items * 8  # clFFT: whole 1024-point frames
        assert direct or (CHUNKS[path] - 1) << 20 < sized <= CHUNKS[path] << 20
    if block == "clMathOp":
        a, b = crandn(rng, items), crandn(rng, items)
        outs, ref = [_host_out(items, np.complex64)], [oracle.mathop(oracle.DTYPE_COMPLEX, oracle.OP_MULTIPLY, a, b)]
        gpu.clMathOp(gpu.DTYPE_COMPLEX, *GPU_ARGS, gpu.MATHOP_MULTIPLY).work(items, [a, b], [outs[0][1]])
    elif block == "clMathConst":
        a = crandn(rng, items)
        outs, ref = [_host_out(items, np.complex64)], [oracle.mathconst(oracle.DTYPE_COMPLEX, oracle.OP_ADD, 1.5, a)]
        gpu.clMathConst(gpu.DTYPE_COMPLEX, *GPU_ARGS, 1.5, gpu.MATHOP_ADD).work(items, [a], [outs[0][1]])
    elif block == "clFFT":
        n = 1024
        nvec = items // n
        x = crandn(rng, nvec * n)
        w = oracle.window(oracle.WIN_BLACKMAN_HARRIS, n)
        outs, ref = [_host_out(nvec * n, np.complex64)], [oracle.fft_block(n, True, w, True, oracle.DTYPE_COMPLEX, x, f64=True)]
        gpu.clFFT(n, gpu.CLFFT_FORWARD, w, gpu.DTYPE_COMPLEX, *GPU_ARGS, 0, 1, True).work(nvec, [x], [outs[0][1]])
    elif block == "clFilter":
        taps = oracle.firdes_low_pass(1.0, 10e6, 1e6, 372000.0)
        inb = (items * 2 + taps.size - 1) * 8  # mi355_filter_work: direct when the call's input fits
        assert (inb <= DIRECT) == direct and (direct or items * 16 // 6 <= 1 << 20 < items * 16 // 3)
        assert direct or (CHUNKS[path] - 1) << 20 < items * 16 <= CHUNKS[path] << 20
        xh = crandn(rng, items * 2 + taps.size - 1)
        outs, ref = [_host_out(items, np.complex64)], [oracle.fir_ccf(taps, xh, items, 2)]
        gpu.clFilter(*GPU_ARGS, 2, taps).work(items, [xh], [outs[0][1]])
    elif block == "clPolyphaseChannelizer":
        M = 64
        buf = items // M * M
        assert ((buf - M + M * 32) * 8 <= DIRECT) == direct  # mi355_pfb_work: the larger of input and output
        taps = (rng.standard_normal(M * 32) / np.sqrt(32)).astype(np.float32)
        blk = gpu.clPolyphaseChannelizer(*GPU_ARGS, taps, buf, M, M, list(range(M)))
        xh = crandn(rng, blk.ninput())
        outs, ref = [_host_out(blk.noutput(), np.complex64)], [oracle.pfb(taps, buf, M, M, list(range(M)), xh, f64=True)]
        blk.general_work(blk.noutput(), [xh.size], [xh], [outs[0][1]])
    elif block == "clComplexToMagPhase":
        assert ((items + 1) * 8 <= DIRECT) == direct
        z = crandn(rng, items)
        outs, ref = [_host_out(items, np.float32), _host_out(items, np.float32, lead=1)], oracle.elem(5, items, [z])
        gpu.clComplexToMagPhase(*GPU_ARGS).work(items, [z], [outs[0][1], outs[1][1]])
    else:
        n = 256
        nfr = items // n
        assert ((nfr * n * 8 * 3 > 64 << 20) == (path == "two_staged_chunks")) and nfr * n * 8 * 3 < 128 << 20
        ins = [crandn(rng, nfr * n) for _ in range(3)]
        outs, ref = [_host_out(nfr * n, np.float32), _host_out(nfr * n, np.float32, lead=1)], oracle.xcorr_fft(n, 2, ins, use_f64=True)
        ocl, sel, plat, dev = GPU_ARGS
        gpu.clxcorrelate_fft_vcf(n, 3, ocl, sel, plat, dev, 2).work(nfr, ins, [outs[0][1], outs[1][1]])
    for (whole, view, lo), r in zip(outs, ref):
        _host_check(whole, lo, view.size)
        assert relerr(view, r) <= TOL


# ------------------------------------------------------------------------------------------------------------- the refusals

def _refused(gpu, call, outs):
    """the call raises Mi355Error and launches nothing: the outputs still hold their pre-fill"""
    with pytest.raises(gpu.Mi355Error):
        call()
    torch.cuda.synchronize()
    for whole, view in outs:
        g = whole._guard
        assert not torch.isfinite(torch.view_as_real(view) if view.is_complex() else view).any(), "a refused call wrote its output"
        assert torch.equal(whole[:g["start"]].view(torch.int32), torch.full((g["start"] // 4,), SENTINEL, dtype=torch.int32, device=DEV))


def test_refusals_four_byte_aligned_buffers(gpu, oracle):
    """a float32 view one float past a 16-byte boundary is 4-byte aligned only: clFFT with real input, clFilter and the channelizer
    refuse it (on either side)"""
    n, nvec = 256, 5
    fft = gpu.clFFT(n, gpu.CLFFT_FORWARD, [], gpu.DTYPE_FLOAT, *GPU_ARGS, 0, 1, False)
    _, x = guarded_input(np.ones(nvec * n, np.float32), pad_items(4), 1, DEV)
    yw, y = guarded_output(nvec * n, np.complex64, pad_items(8), 0, DEV)
    _refused(gpu, lambda: fft.work_device(nvec, [x], [y]), [(yw, y)])
    flt = gpu.clFilter(*GPU_ARGS, 1, np.ones(9, np.float32), 1, 0, False)
    nout = 1000
    _, xf = guarded_input(np.ones(2 * (nout + 8), np.float32), pad_items(4), 1, DEV)  # the complex items seen through a float view
    _refused(gpu, lambda: flt.work_device(nout, [xf], [y]), [(yw, y)])
    fw, yf = guarded_output(2 * nout, np.float32, pad_items(4), 1, DEV)
    _, xc = guarded_input(np.ones(nout + 8, np.complex64), pad_items(8), 0, DEV)
    _refused(gpu, lambda: flt.work_device(nout, [xc], [yf]), [(fw, yf)])
    M = 16
    pfb = gpu.clPolyphaseChannelizer(*GPU_ARGS, np.ones(M * 4, np.float32), M * 50, M, M, list(range(M)))
    _, xp = guarded_input(np.ones(2 * pfb.ninput(), np.float32), pad_items(4), 1, DEV)
    pw, yp = guarded_output(pfb.noutput(), np.complex64, pad_items(8), 0, DEV)
    _refused(gpu, lambda: pfb.work_device([xp], [yp]), [(pw, yp)])
    _refused(gpu, lambda: pfb.work_device([xp], [yp], nbuf=1), [(pw, yp)])
    _, xp3 = guarded_input(np.ones(2 * (pfb.ninput() + 2 * M * 50), np.float32), pad_items(4), 1, DEV)
    pw3, yp3 = guarded_output(3 * pfb.noutput(), np.complex64, pad_items(8), 0, DEV)
    _refused(gpu, lambda: pfb.work_device([xp3], [yp3], nbuf=3), [(pw3, yp3)])


@pytest.mark.parametrize("n", [8192, 16384, 15360, 65536])
def test_refusals_eight_byte_aligned_input_of_a_long_transform(gpu, n):
    """lengths above 4096 that are not chirp-z lengths want a 16-byte aligned input (the accepted side, an 8-byte aligned OUTPUT at
    these lengths, is in test_clfft_stays_inside_its_buffers)"""
    fft = gpu.clFFT(n, gpu.CLFFT_FORWARD, [], gpu.DTYPE_COMPLEX, *GPU_ARGS, 0, 1, False)
    _, x = guarded_input(np.ones(2 * n, np.complex64), pad_items(8, n), 1, DEV)
    yw, y = guarded_output(2 * n, np.complex64, pad_items(8, n), 0, DEV)
    _refused(gpu, lambda: fft.work_device(2, [x], [y]), [(yw, y)])


def test_refusals_mathop_and_mathconst_want_sixteen_bytes(gpu):
    n = 1000
    op = gpu.clMathOp(gpu.DTYPE_COMPLEX, *GPU_ARGS, gpu.MATHOP_ADD)
    const = gpu.clMathConst(gpu.DTYPE_COMPLEX, *GPU_ARGS, 2.0, gpu.MATHOP_MULTIPLY)
    one = np.ones(n, np.complex64)
    for oa, ob, oc in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        (_, a), (_, b) = guarded_input(one, pad_items(8), oa, DEV), guarded_input(one, pad_items(8), ob, DEV)
        cw, c = guarded_output(n, np.complex64, pad_items(8), oc, DEV)
        _refused(gpu, lambda: op.work_device(n, [a, b], [c]), [(cw, c)])
        if not ob:
            _refused(gpu, lambda: const.work_device(n, [a], [c]), [(cw, c)])


def test_refusals_short_tensors_of_the_fft_correlator(gpu):
    """work_device() of clxcorrelate_fft_vcf checks every tensor against nframes x fft_size items (complex64 in, float32 out): a short one
    is a ValueError before anything is launched, not a device memory fault"""
    n, nfr = 256, 5
    ocl, sel, plat, dev = GPU_ARGS
    blk = gpu.clxcorrelate_fft_vcf(n, 3, ocl, sel, plat, dev, 2)
    ins = [guarded_input(np.ones(nfr * n, np.complex64), pad_items(8, n), 0, DEV)[1] for _ in range(3)]
    outs = [guarded_output(nfr * n, np.float32, pad_items(4, n), 0, DEV) for _ in range(2)]
    ov = [v for _, v in outs]
    for bad_in, bad_out in ((2, None), (0, None), (None, 1), (None, 0)):
        i = [x[:-1] if k == bad_in else x for k, x in enumerate(ins)]
        o = [y[:-1] if k == bad_out else y for k, y in enumerate(ov)]
        with pytest.raises(ValueError, match="holds %d bytes" % ((nfr * n - 1) * (8 if bad_out is None else 4))):
            blk.work_device(nfr, i, o)
    with pytest.raises(ValueError):
        blk.work_device(nfr, ins[:2], ov)
    torch.cuda.synchronize()
    for whole, view in outs:
        assert not torch.isfinite(view).any(), "a refused call wrote its output"
        check_guards(whole, view, interior=False)
    blk.work_device(nfr, ins, ov)  # exactly the items: accepted
    torch.cuda.synchronize()
    for whole, view in outs:
        check_guards(whole, view)
