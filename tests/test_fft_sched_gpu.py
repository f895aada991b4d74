"""GPU: the persistent clFFT schedule with dynamic frame-group claims (MI355_FFT_SCHED=1; the default at 4096 points) gives bit for
bit what the static grid stride (MI355_FFT_SCHED=0; the default below 4096 points) gives: both run the same arithmetic per frame,
only the workgroup that does a frame differs.  The claim words reset themselves at the end of every launch, and every stream that
calls a handle gets a word set of its own, so back-to-back launches, one handle on several streams at once and several handles at
once must all stay exact.  Every concurrent test below forces the claim schedule and fills its outputs with NaN first, so a group
that a broken claim word skipped shows up."""
import os

import numpy as np
import pytest

from conftest import GPU_ARGS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _frames(n, extra_groups):
    """Frame count whose last group is ragged: the persistent path starts at 16 groups per CU (two workgroups of >= 8 groups)."""
    f = max(4096 // n, 1)  # frames per group
    return (_cus() * 16 + extra_groups - 1) * f + (f // 2 + 1 if f > 1 else 1)


def _blk(gpu, n, fwd=True, shift=True, real=False, window=True):
    w = np.blackman(n).astype(np.float32) if window else []
    return gpu.clFFT(n, gpu.CLFFT_FORWARD if fwd else gpu.CLFFT_BACKWARD, w, gpu.DTYPE_FLOAT if real else gpu.DTYPE_COMPLEX,
                     *GPU_ARGS, 0, 1, shift)


def _input(n, frames, real, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if real:
        return torch.randn(frames * n, device="cuda", generator=g)
    return torch.randn(frames * n, 2, device="cuda", generator=g)


def _run(blk, n, frames, x, sched):
    os.environ["MI355_FFT_SCHED"] = str(sched)
    try:
        y = torch.full((frames * n, 2), float("nan"), device="cuda")
        blk.work_device(frames, [x], [y])
        torch.cuda.synchronize()
        return y
    finally:
        os.environ.pop("MI355_FFT_SCHED", None)


def _nan_out(n, frames):
    return torch.full((frames * n, 2), float("nan"), device="cuda")


class _Sched:
    """MI355_FFT_SCHED set for the launches inside the block (it is read per call)"""

    def __init__(self, v):
        self.v = str(v)

    def __enter__(self):
        os.environ["MI355_FFT_SCHED"] = self.v

    def __exit__(self, *exc):
        os.environ.pop("MI355_FFT_SCHED", None)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", [16, 64, 256, 1024, 4096])
@pytest.mark.parametrize("mode", ["fwd_shift", "rev_shift", "fwd", "rev", "real_fwd_shift"])
@pytest.mark.parametrize("extra", [0, 37])
def test_dynamic_equals_static(gpu, n, mode, extra):
    fwd, shift, real = mode.startswith(("fwd", "real")), mode.endswith("shift"), mode.startswith("real")
    frames = _frames(n, extra)
    blk = _blk(gpu, n, fwd, shift, real)
    x = _input(n, frames, real, 1000 * n + extra)
    a = _run(blk, n, frames, x, 0)
    b = _run(blk, n, frames, x, 1)
    assert _same(a, b)
    assert torch.isfinite(b).all()
    c = _run(blk, n, frames, x, 1)  # the words were reset by the launch before
    assert _same(a, c)


def test_dynamic_matches_numpy(gpu):
    n = 4096
    frames = _frames(n, 5)
    blk = _blk(gpu, n)
    x = _input(n, frames, False, 77)
    y = _run(blk, n, frames, x, 1)
    w = np.blackman(n)
    idx = [0, 1, frames // 2, frames - 2, frames - 1]
    xc = x.view(frames, n, 2).cpu().numpy()[idx].astype(np.float64)
    ref = np.fft.fftshift(np.fft.fft((xc[..., 0] + 1j * xc[..., 1]) * w, axis=1), axes=1)
    got = y.view(frames, n, 2).cpu().numpy()[idx]
    got = got[..., 0] + 1j * got[..., 1]
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
    from fft_ref import fft_bound_check, fft_bound_kind
    assert blk.last_route() == "k_fft<4096> PF=1 dyn grid=%d" % (2 * _cus())
    fft_bound_check(got.astype(np.complex64), ref, n, fft_bound_kind(blk.last_route()))


@pytest.mark.parametrize("n,default", [(4096, "1"), (1024, "0")])
def test_default_schedule(gpu, tmp_path, n, default):
    """at the smallest persistent frame count, 4096 points take the claim schedule by default and shorter transforms the static
    one (stamps record the schedule of a launch); MI355_FFT_SCHED overrides it either way"""
    frames = _frames(n, 0)
    blk = _blk(gpu, n)
    x = _input(n, frames, False, 5)
    y = torch.empty(frames * n, 2, device="cuda")
    path = str(tmp_path / "stamps.txt")
    other = "0" if default == "1" else "1"
    os.environ.update({"MI355_FFT_TS": "1", "MI355_FFT_TS_FILE": path})
    try:
        blk.work_device(frames, [x], [y])
        os.environ["MI355_FFT_SCHED"] = other
        blk.work_device(frames, [x], [y])
        torch.cuda.synchronize()
    finally:
        for k in ("MI355_FFT_TS", "MI355_FFT_TS_FILE", "MI355_FFT_SCHED"):
            os.environ.pop(k, None)
    heads = [line.split() for line in open(path) if line.startswith("#")]
    assert [h[h.index("sched") + 1] for h in heads] == [default, other]
    rows = [list(map(int, line.split()[:5])) for line in open(path) if not line.startswith("#")]
    grid = int(heads[0][heads[0].index("grid") + 1])
    ngroups = int(heads[0][heads[0].index("ngroups") + 1])
    assert sum(r[4] for r in rows[:grid]) == ngroups  # every group done exactly once, by either schedule
    assert sum(r[4] for r in rows[grid:]) == ngroups


def test_back_to_back_launches(gpu):
    """50 launches in a row on one handle and stream, each into its own output: the claim words reset themselves"""
    n = 4096
    frames = _frames(n, 3)
    blk = _blk(gpu, n)
    xs = [_input(n, frames, False, 300 + i) for i in range(2)]
    refs = [_run(blk, n, frames, x, 0) for x in xs]
    ys = [_nan_out(n, frames) for _ in range(50)]
    with _Sched(1):
        for i, y in enumerate(ys):
            blk.work_device(frames, [xs[i % 2]], [y])
        torch.cuda.synchronize()
    assert all(_same(y, refs[i % 2]) for i, y in enumerate(ys))


@pytest.mark.parametrize("n", [1024, 4096])
def test_one_handle_two_streams(gpu, n):
    """one handle, launches in flight on two streams at once, both with claims: each stream must use its own word set"""
    frames = _frames(n, 11)
    blk = _blk(gpu, n)
    xs = [_input(n, frames, False, 500 + i) for i in range(2)]
    refs = [_run(blk, n, frames, x, 0) for x in xs]
    streams = [torch.cuda.Stream() for _ in range(2)]
    ys = [[_nan_out(n, frames) for _ in range(8)] for _ in range(2)]
    torch.cuda.synchronize()
    with _Sched(1):
        for k in range(8):
            for s in range(2):
                with torch.cuda.stream(streams[s]):
                    blk.work_device(frames, [xs[s]], [ys[s][k]])
        torch.cuda.synchronize()
    assert all(_same(y, refs[s]) for s in range(2) for y in ys[s])
    # and the words of both sets were left at zero: one more launch on each stream, then on the default stream
    with _Sched(1):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                ys[s][0].fill_(float("nan"))
                blk.work_device(frames, [xs[s]], [ys[s][0]])
        torch.cuda.synchronize()
    assert all(_same(ys[s][0], refs[s]) for s in range(2))
    assert _same(_run(blk, n, frames, xs[0], 1), refs[0])


def test_two_handles_two_streams(gpu):
    n = 4096
    frames = _frames(n, 1)
    blks = [_blk(gpu, n), _blk(gpu, n, fwd=False, shift=False)]
    x = _input(n, frames, False, 900)
    refs = [_run(b, n, frames, x, 0) for b in blks]
    streams = [torch.cuda.Stream() for _ in range(2)]
    ys = [[_nan_out(n, frames) for _ in range(6)] for _ in range(2)]
    torch.cuda.synchronize()
    with _Sched(1):
        for k in range(6):
            for s in range(2):
                with torch.cuda.stream(streams[s]):
                    blks[s].work_device(frames, [x], [ys[s][k]])
        torch.cuda.synchronize()
    assert all(_same(y, refs[s]) for s in range(2) for y in ys[s])


# ---- one handle's workspace on two streams ---------------------------------------------------------------------------------------
# length, create-time switch, what mi355_fft_plan_text says of the length, the start of last_route()
WORKSPACE_ROUTES = [
    (65536, None, "two tile passes 256 x 256", "k_fft_tile 256x256"),
    (131072, "MI355_FFT_NO_TILE", "two tile passes 256 x 512", "k_fft_sub+combine2 S=16x2"),  # three passes: both workspace halves
    (20000, None, "mixed radix, two passes", "k_fft_mr_tile"),
    (8209, None, "chirp-z, m = 32768", "bluestein m=32768"),                                   # the unfused five-launch path
]


def _plan_text(gpu, n):
    import ctypes
    b = ctypes.create_string_buffer(200)
    assert gpu.lib().mi355_fft_plan_text(n, b, 200) == 0
    return b.value.decode()


@pytest.mark.parametrize("n,switch,plan,route", WORKSPACE_ROUTES)
def test_one_handle_two_streams_workspace(gpu, monkeypatch, n, switch, plan, route):
    """the routes that go through the handle's workspace: 6 calls per stream on two streams in turn with nothing waited for in
    between, the first of 1 frame and the others of 3, so the workspace grows after it has been used and is handed from stream to
    stream 11 times.  Every NaN-filled output is bit for bit what a second handle gives for the same input on one stream."""
    if switch:
        monkeypatch.setenv(switch, "1")  # read at create
    assert _plan_text(gpu, n).startswith(plan)  # (the default plan: plan_text honours no switch)
    blk, single = _blk(gpu, n), _blk(gpu, n)
    xs = [_input(n, 3, False, 700 + n % 97 + i) for i in range(2)]
    frames = lambda k, s: 1 if (k, s) == (0, 0) else 3  # noqa: E731
    refs = {}
    for s in range(2):
        for f in (1, 3):
            refs[s, f] = _nan_out(n, f)
            single.work_device(f, [xs[s][:f * n]], [refs[s, f]])
            torch.cuda.synchronize()
    assert single.last_route().startswith(route), single.last_route()
    streams = [torch.cuda.Stream() for _ in range(2)]
    ys = [[_nan_out(n, frames(k, s)) for k in range(6)] for s in range(2)]
    torch.cuda.synchronize()
    for k in range(6):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                blk.work_device(frames(k, s), [xs[s][:frames(k, s) * n]], [ys[s][k]])
    torch.cuda.synchronize()
    assert blk.last_route().startswith(route), blk.last_route()
    for s in range(2):
        for k in range(6):
            assert torch.isfinite(ys[s][k]).all(), (s, k)
            assert _same(ys[s][k], refs[s, frames(k, s)]), (s, k)
