"""GPU: every route of clFFT held to the per-frame error bounds of tests/fft_ref.py (fft_bound_check against the float64 fft_frames64; the
multiples are fixed on the CPU by tests/test_fft_ref.py), to the route it is named for (clFFT.last_route()), and to frame-local reach.

One case per route at the smallest shapes that take it.  Every call runs on the device path into an output filled with NaN.  Inputs
(fft_ref.fft_inputs): `mixed` -- noise frames scaled by 10^U(-3, 3) per frame with two all-zero frames, one of them the last frame of the
ragged last group, which must come out as exact zeros; `impulses` -- the identity for n <= 1024 (the output is the whole DFT matrix), edge
and seeded positions above; `tones` -- one per bin for n <= 1024, edge and seeded bins above, built in float64 and rounded, compared
with the float64 transform of the rounded input; `tone_noise` -- the tones plus noise at -60 dB.  The persistent cases carry the three
special kinds inside their one large call; lengths above 65536 run them with the frame count of the case.

Reach: one non-finite item (NaN in both components, NaN for real input) in the first item of a frame, the last item of a frame, a frame
of the ragged last group and, for the persistent cases, a frame of a group that is claimed dynamically.  Every bin of that frame must be
non-finite (complex input: both components; real input: some component), every other frame must have the bits of the clean call.
include/mi355_clenabled.h states the contract.

Every test prints `USED <route label> ...` lines with the used fraction of each bound (pytest -s); DESIGN.md, 'Tolerances', records them."""
import re

import numpy as np
import pytest
import torch

from conftest import GPU_ARGS
from fft_ref import MR_PLANS, MR_TILE_PLANS, fft_bound_check, fft_frames64, fft_inputs
from test_device_bounds_gpu import MODES
from test_fft_sched_gpu import _cus, _frames

pytestmark = pytest.mark.gpu

SMALL = ["fwd_shift_win", "bwd_shift", "fwd", "real_fwd_shift_win"]
BIG = ["fwd_shift_win", "bwd"]  # the persistent-sized calls and 2^21 points and more: both directions, the shift on and off (as the guard-band grid)
KINDS = ["mixed", "impulses", "tones", "tone_noise"]
CASES = []


def _add(label, n, frames, modes, route, env=None, bound="direct", split_kinds=False):
    """route: the text last_route() must give (a string, `{cus2}` = two workgroups per CU), or a function of the text"""
    tag = "".join("-%s=%s" % (k.replace("MI355_FFT_", ""), v) for k, v in (env or {}).items())
    for m in modes:
        for kinds in ([(k,) for k in KINDS] if split_kinds else [tuple(KINDS)]):
            ident = "%s%s-n%d-frames_%s-%s%s" % (label, tag, n, frames, m, "-" + kinds[0] if split_kinds else "")
            CASES.append(pytest.param(label, n, frames, m, env or {}, route, bound, kinds, id=ident))


def _mr(n, variant, threads=None, frames=None):
    """exactly the plan of this variant (MR_PLANS[n]: the rule's factorisation first, the alternative one last; tests/test_fft_ref.py emulates
    both, the mixed-radix multiples were fixed on those), and the pinned workgroup shape if any.  Every case of a length with two plans pins
    MI355_FFT_MR_VARIANT, so what it runs does not depend on the handles the process made before."""
    plan = MR_PLANS[n][-1 if variant else 0]
    assert variant is not None or len(MR_PLANS[n]) == 1

    def ok(text):
        m = re.fullmatch(r"k_fft_mr (\d+(?:x\d+)*) threads=(\d+) frames=(\d+)", text)
        return bool(m) and tuple(int(r) for r in m.group(1).split("x")) == plan and \
            (threads is None or (int(m.group(2)), int(m.group(3))) == (threads, frames))
    return ok


def _mr_tile(n):
    n1, n2, ra, rb = MR_TILE_PLANS[n]
    return "k_fft_mr_tile %d x %d (%s, %s)" % (n1, n2, "x".join(map(str, ra)), "x".join(map(str, rb)))


for _n in (2, 8, 64):
    _g = 4096 // _n
    for _fr in (3 * _g - 1, 3 * _g + 1):
        _add("lds_redistributed", _n, _fr, SMALL, "k_fft<%d> PF=0" % _n)
for _n in (128, 1024, 4096):
    _g = 4096 // _n
    _add("grid_stride", _n, 3 * _g + 1, SMALL, "k_fft<%d> PF=0" % _n)
for _m in BIG:  # (the per-call switches innermost: consecutive cases share input and reference)
    _add("persistent", 16, "persistent+37", [_m], "k_fft<16> PF=1 static grid={cus2}")
    _add("persistent", 1024, "persistent+37", [_m], "k_fft<1024> PF=1 static grid={cus2}")
    _add("persistent", 4096, "persistent+37", [_m], "k_fft<4096> PF=1 dyn grid={cus2}")
    _add("persistent", 4096, "persistent+37", [_m], "k_fft<4096> PF=1 static grid={cus2}", {"MI355_FFT_SCHED": "0"})
    _add("persistent", 4096, "persistent+37", [_m], "k_fft<4096> PF=1 dyn grid={cus2}", {"MI355_FFT_SCHED": "1"})
    _add("persistent_sized", 4096, "persistent+37", [_m], "k_fft<4096> PF=0", {"MI355_FFT_PREFETCH": "0"})
    _add("persistent_sized", 4096, "persistent+37", [_m], "k_fft<4096> PF=2", {"MI355_FFT_PREFETCH": "2"})
for _n in (8192, 16384):
    _add("k_fft_s", _n, 3, SMALL, "k_fft_s<%d>" % _n)
_add("k_fft_32k", 32768, 3, SMALL, "k_fft_32k")
# (256x256 on the impulse set uses 0.98 of the per-bin bound -- its W_N^(n2 k1) is a product of table entries; DESIGN.md, 'Tolerances'.  The
# set is seeded (fft_ref.impulse_positions): another seed or position list can move it past 1, which is then this known figure, not a new fault)
for _n, _t in ((65536, "256x256"), (131072, "256x512"), (1 << 20, "1024x1024")):
    _add("tile_passes", _n, 2, SMALL, "k_fft_tile " + _t)
for _lg in (21, 22, 23, 24):  # the last combine is radix 2, 4, 8, 16
    _add("four_passes", 1 << _lg, 1, BIG, "k_fft_sub+combine2 S=16x16x%d" % (1 << (_lg - 20)), split_kinds=True)
for _n in (12, 96):
    for _v in ("0", "1"):
        _add("mixed_radix", _n, 11, SMALL, _mr(_n, int(_v)), {"MI355_FFT_MR_VARIANT": _v}, bound="mixed_radix")
assert MR_PLANS[96][0] != MR_PLANS[96][-1] and MR_PLANS[1000][0] != MR_PLANS[1000][-1]  # two factorisations, two roundings
for _v in ("0", "1"):  # 10x10x10 and 5x5x5x8
    _add("mixed_radix", 1000, 11, SMALL, _mr(1000, int(_v)), {"MI355_FFT_MR_VARIANT": _v}, bound="mixed_radix")
for _n in (3840, 13312, 15360):  # (one plan each)
    _add("mixed_radix", _n, 11, SMALL, _mr(_n, None), bound="mixed_radix")
for _t, _f in ((256, 1), (512, 3)):  # frames per iteration pinned: the case does not depend on a timing
    _add("mixed_radix", 1000, 11, SMALL, _mr(1000, 0, _t, _f),
         {"MI355_FFT_MR_VARIANT": "0", "MI355_FFT_MR_AUTOTUNE": "0", "MI355_FFT_MR_THREADS": str(_t), "MI355_FFT_MR_FRAMES": str(_f)},
         bound="mixed_radix")
for _n in (16000, 22050, 921600):
    _add("mixed_radix_two_passes", _n, 2, SMALL, _mr_tile(_n), bound="mixed_radix_two_passes")
_add("chirpz_fused", 4099, 7, SMALL, "k_chirpz<16384>", bound="chirpz")
_add("chirpz_fused", 1200, 7, SMALL, "k_chirpz<4096>", {"MI355_FFT_NO_MR": "1"}, bound="chirpz")
# (16383: m = 32768, one pass inside; 16385: m = 65536 and 100003: m = 262144, the two tile passes inside, through handles of their own)
for _n, _t in ((16383, "bluestein m=32768: k_fft_32k"), (16385, "bluestein m=65536: k_fft_tile 256x256"),
               (100003, "bluestein m=262144: k_fft_tile 512x512")):
    _add("chirpz_unfused", _n, 2, SMALL, _t, bound="chirpz")


def _special_frames(n):
    """frames of the impulse and tone sets: the identity plus one for n <= 1024, 64 up to 65536 points, the case's own count above"""
    return n + 1 if n <= 1024 else 64 if n <= 65536 else 0


def _window(n):
    return np.hamming(n).astype(np.float32)


_DATA = {}


def _data(n, frames, mode, kind, embed):
    """(input (frames, n), float64 reference) of one call; kept for the next case when only a switch differs.  embed: the persistent
    cases -- the special kinds ride inside the mixed call, spread over its frames."""
    key = (n, frames, mode, kind, embed)
    if key not in _DATA:
        _DATA.clear()
        fwd, shift, win, real = MODES[mode]
        seed = 7 * n + frames + KINDS.index(kind)
        x = fft_inputs(kind, n, frames, seed, real)
        if embed:
            k = _special_frames(n)
            for i, other in enumerate(KINDS[1:]):
                at = (np.arange(k) * (frames // k) + 1 + i) % frames
                at = at[(at != frames - 1) & (at != frames // 2)]  # (the zero frames stay)
                x[at] = fft_inputs(other, n, k, seed + 1 + i, real)[:len(at)]
        _DATA[key] = (x, fft_frames64(n, fwd, _window(n) if win else None, shift, x, real))
    return _DATA[key]


def _blk(gpu, n, mode):
    fwd, shift, win, real = MODES[mode]
    return gpu.clFFT(n, gpu.CLFFT_FORWARD if fwd else gpu.CLFFT_BACKWARD, _window(n) if win else [], gpu.DTYPE_FLOAT if real else gpu.DTYPE_COMPLEX,
                     *GPU_ARGS, 0, 1, shift)


def _dev(x):
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return torch.view_as_real(t) if t.is_complex() else t


def _call(blk, n, frames, xd):
    y = torch.full((frames, n, 2), float("nan"), device="cuda")
    blk.work_device(frames, [xd], [y])
    torch.cuda.synchronize()
    return y


def _host(y):
    return np.ascontiguousarray(y.cpu().numpy().view(np.complex64)[..., 0])


def _check_route(blk, route):
    text = blk.last_route()
    if callable(route):
        assert route(text), text
    else:
        assert text == route.format(cus2=2 * _cus()), text
    return text


def _nframes(n, frames):
    if isinstance(frames, str):
        frames = _frames(n, int(frames.split("+")[1]))
        assert (frames + max(4096 // n, 1) - 1) // max(4096 // n, 1) >= _cus() * 16
    return frames


@pytest.mark.parametrize("label,n,frames,mode,env,route,bound,kinds", CASES)
def test_clfft_bounds_and_route(gpu, monkeypatch, label, n, frames, mode, env, route, bound, kinds):
    embed = isinstance(frames, str)
    frames = _nframes(n, frames)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blk = _blk(gpu, n, mode)
    assert blk.last_route() == ""
    for kind in (["mixed"] if embed else kinds):
        # the special sets of a short length are longer than the case (the identity); they must still take the route of the case
        nf = frames if kind == "mixed" or embed else (_special_frames(n) or frames)
        x, ref = _data(n, nf, mode, kind, embed)
        got = _host(_call(blk, n, nf, _dev(x)))
        text = _check_route(blk, route)
        fb, fr = fft_bound_check(got, ref, n, bound, check=False)
        print("USED %s | %s | n %d frames %d %s %s: bin %.3f rss %.3f" % (label, text, n, nf, mode, kind, fb, fr))
        fft_bound_check(got, ref, n, bound, what="%s %s" % (text, kind))


def _plants(n, frames, persistent):
    """(frame, item) of the planted non-finite items"""
    f = max(4096 // n, 1)
    out = [(min(1, frames - 1), 0), (min(frames // 2 + 1, frames - 1), n - 1), (frames - 1, n // 3)]
    if persistent:
        ngroups = (frames + f - 1) // f
        out.append((f * (ngroups // 8 - 10) + f // 2, 5))  # the end of the first claim class' range: past its workgroups' static groups
    return out


REACH = {}
for _c in CASES:
    _label, _n, _fr, _mode, _env, _route, _bound, _kinds = _c.values
    if _kinds[0] == "mixed":
        REACH[_c.id] = pytest.param(_label, _n, _fr, _mode, _env, _route, id=_c.id.replace("-mixed", ""))


@pytest.mark.parametrize("label,n,frames,mode,env,route", list(REACH.values()))
def test_clfft_reach_is_the_frame(gpu, monkeypatch, label, n, frames, mode, env, route):
    persistent = label == "persistent"
    frames = _nframes(n, frames)
    real = MODES[mode][3]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    blk = _blk(gpu, n, mode)
    xd = _dev(fft_inputs("mixed", n, frames, 3 * n + frames, real))  # (frames, n, 2), or (frames, n) for real input
    clean = _call(blk, n, frames, xd)
    _check_route(blk, route)
    assert torch.isfinite(clean).all()
    plants = _plants(n, frames, persistent)
    calls = [plants] if frames >= 8 else [[p] for p in plants]
    for call in calls:
        xn = xd.clone()
        for f, i in call:
            xn[f, i] = float("nan")
        got = _call(blk, n, frames, xn)
        _check_route(blk, route)
        bad = ~torch.isfinite(got)  # (frames, n, 2)
        other = torch.ones(frames, dtype=torch.bool, device="cuda")
        for f, i in call:
            other[f] = False
            hit = bad[f].any(dim=-1) if real else bad[f].all(dim=-1)
            assert bool(hit.all()), "a non-finite item %d of frame %d left %d bins of its frame finite" % (i, f, int((~hit).sum()))
        same = (got.view(torch.int32) == clean.view(torch.int32)).view(frames, -1).all(dim=1)
        wrong = torch.nonzero(other & ~same).flatten()
        assert wrong.numel() == 0, "a non-finite item in frames %s changed frames %s" % ([f for f, _ in call], wrong[:8].tolist())


def test_host_path_multi_chunk_equals_the_device_path(gpu):
    """work() of 700 frames of 4096 points runs in several chunks through the staging slots: every frame bit for bit what work_device gives"""
    n, frames = 4096, 700
    blk = _blk(gpu, n, "fwd_shift_win")
    x = fft_inputs("mixed", n, frames, 700)
    dev = _host(_call(blk, n, frames, _dev(x)))
    y = np.full(frames * n, np.nan + 0j, np.complex64)
    blk.work(frames, [x.reshape(-1)], [y])
    same = (y.view(np.int32).reshape(frames, -1) == dev.reshape(frames, n).view(np.int32).reshape(frames, -1)).all(axis=1)
    assert same.all(), np.flatnonzero(~same)[:8]
    fb, fr = fft_bound_check(y, fft_frames64(n, True, _window(n), True, x), n)
    print("USED host_path | %s | n %d frames %d: bin %.3f rss %.3f" % (blk.last_route(), n, frames, fb, fr))


def test_host_path_three_real_streams_equal_the_device_path(gpu):
    n, frames = 512, 37
    w = _window(n)
    blk = gpu.clFFT(n, gpu.CLFFT_FORWARD, w, gpu.DTYPE_FLOAT, *GPU_ARGS, 0, 3, True)
    one = gpu.clFFT(n, gpu.CLFFT_FORWARD, w, gpu.DTYPE_FLOAT, *GPU_ARGS, 0, 1, True)
    xs = [fft_inputs(k, n, frames, 512 + i, real=True) for i, k in enumerate(("mixed", "tones", "tone_noise"))]
    ys = [np.full(frames * n, np.nan + 0j, np.complex64) for _ in xs]
    blk.work(frames, [x.reshape(-1) for x in xs], ys)
    for x, y in zip(xs, ys):
        dev = _host(_call(one, n, frames, _dev(x)))
        assert np.array_equal(y.view(np.int32), dev.reshape(-1).view(np.int32))
        fft_bound_check(y, fft_frames64(n, True, w, True, x, real=True), n)
