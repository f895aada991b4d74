"""GPU: clPowerSpectrum against tests/pspec_ref.py (float64, rounded to float).  One tolerance for linear output, conftest.relerr <=
ref.TOL = 1e-5 (DESIGN.md "Tolerances"); every output of every case is compared; the output is NaN before every call.

Routes, as csrc/pspec.hip states them:
  fused pow2   N = 16 .. 4096 a power of two; a frame group is F = 4096 / N frames, a chunk C = max(64, 16 F) frames (route() names it);
               K <= C: one kernel; K > C: partial sums per chunk and a second kernel
  generic      every other length clFFT takes (8192 and up, mixed radix, chirp-z) and every handle under set_generic(True): frames in
               batches (route() names the batch) through an internal clFFT, then one sum per bin
"""
import re
import threading

import numpy as np
import pytest

from conftest import GPU_ARGS, relerr
import guarded
import pspec_ref as ref

pytestmark = pytest.mark.gpu
FUSED_NS = (16, 64, 256, 1024, 4096)  # 4096 is the largest fused length
GENERIC_NS = (12, 100, 1000, 4099, 32768)


def chunk_of(route):
    m = re.search(r"(?:chunk|batch)=(\d+)", route)
    return int(m.group(1))


def _run(blk, d_x, S, N):
    """work_device on a NaN-filled output"""
    import torch
    d_out = torch.full((max(S * N, 1),), float("nan"), dtype=torch.float32, device="cuda")
    assert blk.work_device(S, [d_x], [d_out]) == S * N
    return d_out.cpu().numpy()[:S * N].reshape(S, N)


def _hops(N):
    return (N, N // 2, N + 5, 3)


@pytest.mark.parametrize("N", FUSED_NS)
def test_grid(gpu, N):
    """K in {1, 2, 3, C-1, C, C+1, 2C+3}, H rotating over {N, N/2, N+5, 3}, S in {1, 2, 5} on the prefix of one stream (the spectra of
    a shorter call are a prefix of the longer one's); Hann / no window and shift alternate"""
    import torch
    probe = gpu.clPowerSpectrum(*GPU_ARGS, N, 1)
    C = chunk_of(probe.route())
    probe.stop()
    assert C % (4096 // N) == 0 and C >= 64
    worst = 0.0
    for i, K in enumerate((1, 2, 3, C - 1, C, C + 1, 2 * C + 3)):
        H = _hops(N)[(i + N.bit_length()) % 4]
        w = ref.hann(N) if i % 2 == 0 else None
        shift = (i // 2) % 2 == 1
        blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H, shift)
        assert blk.route() == "fused pow2 N=%d chunk=%d" % (N, C) and blk.history() == max(N - H, 0)
        x = ref.make_input(ref.plan(N, K, H, 5)[0], seed=N + K)
        want = ref.pspec(x, N, K, H, 5, w, shift)
        d_x = torch.from_numpy(x).cuda()
        for S in (1, 2, 5):
            e = relerr(_run(blk, d_x[:ref.plan(N, K, H, S)[0]], S, N), want[:S])
            worst = max(worst, e)
            assert e <= ref.TOL, (N, K, H, S, e)
        blk.stop()
    print("N=%d worst relerr %.3g" % (N, worst))


@pytest.mark.parametrize("S", [1, 3])
def test_long_average(gpu, S):
    import torch
    N, K = 256, 1000
    x = ref.make_input(ref.plan(N, K, N, S)[0], seed=9)
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, ref.hann(N))
    e = relerr(_run(blk, torch.from_numpy(x).cuda(), S, N), ref.pspec(x, N, K, N, S, ref.hann(N)))
    print("N=256 K=1000 S=%d relerr %.3g" % (S, e))
    assert e <= ref.TOL, e
    blk.stop()


@pytest.mark.parametrize("N", GENERIC_NS)
def test_generic_route_lengths(gpu, N):
    """lengths the fused kernel does not take (mixed radix, chirp-z, above 4096 points), at H = N and at one H != N each; odd lengths
    check the shift rule"""
    import torch
    K, S = (3, 2) if N >= 4096 else (9, 3)
    for H, w, shift in ((N, ref.hann(N), True), ({12: 5, 100: 150, 1000: 500, 4099: 4100, 32768: 16384}[N], None, N % 2 == 1)):
        blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H, shift)
        assert blk.route().startswith("generic N=%d" % N)
        x = ref.make_input(ref.plan(N, K, H, S)[0], seed=N)
        e = relerr(_run(blk, torch.from_numpy(x).cuda(), S, N), ref.pspec(x, N, K, H, S, w, shift))
        assert e <= ref.TOL, (N, H, e)
        blk.stop()


def test_generic_route_more_frames_than_a_batch(gpu):
    """K above the batch of the generic route: the sum is carried from batch to batch"""
    import torch
    N = 32768
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, 1)
    B = chunk_of(blk.route())
    blk.stop()
    assert B == 32
    K, S = B + 3, 2
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, None, N, True)
    x = ref.make_input(ref.plan(N, K, N, S)[0], seed=2)
    e = relerr(_run(blk, torch.from_numpy(x).cuda(), S, N), ref.pspec(x, N, K, N, S, None, True))
    assert e <= ref.TOL, e
    blk.stop()


@pytest.mark.parametrize("N,K,S", [(1 << 21, 3, 1), (1 << 23, 1, 2)])
def test_generic_route_above_2_20_points(gpu, N, K, S):
    """above 2^20 points the batch is one frame: K > 1 carries the sum frame by frame, and K = 1 is a batch of whole spectra although
    one spectrum alone passes the 2^22 values such a batch is sized for (2^23 points: one spectrum per batch, two batches)"""
    import torch
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, None, N, True)
    assert blk.route() == "generic N=%d batch=1" % N
    x = ref.make_input(ref.plan(N, K, N, S)[0], seed=K)
    e = relerr(_run(blk, torch.from_numpy(x).cuda(), S, N), ref.pspec(x, N, K, N, S, None, True))
    assert e <= ref.TOL, e
    blk.stop()


def test_general_work_consumes_no_more_than_it_is_given(gpu):
    """hop > fft_size: a spectrum consumes navg * hop items, more than the (navg - 1) * hop + fft_size it reads"""
    N, K, H, S = 64, 3, 100, 4
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, None, H)
    x = ref.make_input(S * K * H)
    y = np.full(S * N, np.nan, np.float32)
    with pytest.raises(ValueError):
        blk.general_work(S, [x.size - 1], [x[:-1]], [y])  # every frame is there, the last skipped items are not
    assert np.all(np.isnan(y))
    assert blk.general_work(S, [x.size], [x], [y]) == (S, S * K * H)
    assert relerr(y.reshape(S, N), ref.pspec(x, N, K, H, S)) <= ref.TOL
    blk.stop()


@pytest.mark.parametrize("N,K,H", [(64, 70, 64), (1024, 5, 512), (4096, 66, 4101)])
def test_fused_shape_forced_generic(gpu, N, K, H):
    import torch
    w = ref.hann(N)
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H, True)
    assert blk.route().startswith("fused pow2")
    x = ref.make_input(ref.plan(N, K, H, 3)[0], seed=K)
    d_x = torch.from_numpy(x).cuda()
    fused = _run(blk, d_x, 3, N)
    blk.set_generic(True)
    assert blk.route().startswith("generic N=%d" % N)
    want = ref.pspec(x, N, K, H, 3, w, True)
    gen = _run(blk, d_x, 3, N)
    assert relerr(gen, want) <= ref.TOL and relerr(fused, want) <= ref.TOL
    blk.set_generic(False)
    assert blk.route().startswith("fused pow2")
    assert np.array_equal(_run(blk, d_x, 3, N).view(np.uint32), fused.view(np.uint32))
    blk.stop()


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
@pytest.mark.parametrize("N,above", [(1024, False), (1024, True), (16, True), (4096, True)])
def test_any_split_gives_the_same_bits(gpu, N, above, generic):
    """7 spectra as one call, 3 + 4 and 1 + 1 + 5, the input at a 16-byte boundary and one item past it; K below and above the chunk
    (the generic route of the same shape: its sum is one chain whatever K)"""
    import torch
    C = 64 if N >= 1024 else 4096
    K = C + 5 if above else 7
    if N == 16:
        K = C + 300
    H = N // 2 if N == 1024 else N
    S = 7
    w = ref.hann(N)
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H)
    assert chunk_of(blk.route()) == C
    blk.set_generic(generic)
    assert blk.route().startswith("generic" if generic else "fused")
    x = ref.make_input(ref.plan(N, K, H, S)[0], seed=N)
    want = ref.pspec(x, N, K, H, S, w)
    first = None
    for off in (0, 1):
        _, d_x = guarded.guarded_input(x, 16, off, device="cuda")
        assert d_x.data_ptr() % 16 == 8 * off
        for split in ((7,), (3, 4), (1, 1, 5)):
            d_out = torch.full((S * N,), float("nan"), dtype=torch.float32, device="cuda")
            done = 0
            for n in split:
                src = d_x[done * K * H:done * K * H + ref.plan(N, K, H, n)[0]]  # in += S K H
                assert blk.work_device(n, [src], [d_out[done * N:(done + n) * N]]) == n * N
                done += n
            got = d_out.cpu().numpy().reshape(S, N)
            if first is None:
                first = got
                assert relerr(got, want) <= ref.TOL
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), (off, split)
    blk.stop()


BOUNDS = [  # N, K, H, generic
    (1024, 7, 1024, False),    # K no multiple of the 4 frames of a group
    (1024, 67, 512, False),    # the same above the chunk, overlapping frames
    (16, 300, 16, False),      # 256 frames share a group
    (16, 4096 + 9, 16, False),
    (256, 5, 300, False),      # H > N: the gaps are NaN
    (4096, 66, 4101, False),
    (64, 3, 1000, False),
    (1000, 5, 1000, True),     # generic
    (100, 9, 130, True),       # generic, H > N
    (4096, 3, 4096, True),     # a fused shape forced generic
]


@pytest.mark.parametrize("N,K,H,generic", BOUNDS)
def test_guard_bands_and_alignment(gpu, N, K, H, generic):
    """a call reads exactly (S K - 1) H + N items -- and with H > N nothing between the frames, which hold NaN here -- and writes exactly
    S N floats, at offsets of 0 and 1 item from a 16-byte boundary, with the same bits"""
    import torch
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, ref.hann(N), H, True)
    blk.set_generic(generic or not blk.route().startswith("fused"))
    assert blk.route().startswith("generic" if generic else "fused")
    pad_in, pad_out = guarded.pad_items(8), guarded.pad_items(4)
    for S in (1, 3):
        x = ref.make_input(ref.plan(N, K, H, S)[0], seed=S)
        want = ref.pspec(x, N, K, H, S, ref.hann(N), True)
        if H > N:
            gaps = (np.arange(x.size) % H) >= N
            x = x.copy()
            x[gaps] = complex(np.nan, np.nan)
        res = []
        for off in (0, 1):
            wi, vi = guarded.guarded_input(x, pad_in, off, device="cuda")
            wo, vo = guarded.guarded_output(S * N, np.float32, pad_out, off, device="cuda")
            assert blk.work_device(S, [vi], [vo]) == S * N
            torch.cuda.synchronize()
            guarded.check_guards(wi, vi, "input")
            guarded.check_guards(wo, vo, "output")  # (interior finite: no gap item was read)
            res.append(guarded.to_numpy(vo).reshape(S, N))
            assert relerr(res[-1], want) <= ref.TOL, (S, off)
        assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32)), S
    blk.stop()


def test_misaligned_pointers_are_refused(gpu):
    import torch
    N, K = 64, 4
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K)
    L_ = gpu.lib()
    x = torch.from_numpy(ref.make_input(K * N + 8)).cuda()
    out = torch.full((N + 8,), float("nan"), dtype=torch.float32, device="cuda")
    for din, dout in ((4, 0), (0, 2), (8, 1)):
        rc = L_.mi355_pspec_work_dev(blk._h, 1, x.data_ptr() + din, out.data_ptr() + dout, None)
        assert rc == -1 and b"aligned" in L_.mi355_last_error(), (din, dout)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert L_.mi355_pspec_work_dev(blk._h, 1, x.data_ptr() + 8, out.data_ptr() + 4, None) == 0  # any 8-byte / 4-byte alignment is legal
    torch.cuda.synchronize()
    assert relerr(out[1:N + 1].cpu().numpy(), ref.pspec(x.cpu().numpy()[1:], N, K, N, 1)[0]) <= ref.TOL
    blk.stop()


@pytest.mark.parametrize("N", [64, 1024])
def test_db_output(gpu, N):
    """white noise: with rho = min / max of the linear spectrum, the linear tolerance carried through the logarithm is
    10 / ln 10 * TOL / rho = 4.35 TOL / rho dB; 1e-4 dB more for float log10 on values of at most tens of dB"""
    import torch
    K, S = 16, 2
    x = ref.make_input(ref.plan(N, K, N, S)[0], seed=N)
    lin = ref.pspec64(x, N, K, N, S, ref.hann(N))
    rho = float(lin.min() / lin.max())
    assert rho >= 0.05, rho
    for generic in (False, True):
        blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, ref.hann(N), None, False, True)
        blk.set_generic(generic)
        got = _run(blk, torch.from_numpy(x).cuda(), S, N)
        want = ref.pspec(x, N, K, N, S, ref.hann(N), log_output=True)
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err <= 4.35 * 1e-5 / rho + 1e-4, (generic, err, rho)
        blk.stop()
    # P = 0 gives -inf
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, None, None, False, True)
    got = _run(blk, torch.zeros(K * N, dtype=torch.complex64, device="cuda"), 1, N)
    assert np.all(np.isneginf(got))
    blk.stop()


def test_set_window_between_enqueued_calls(gpu):
    """two work_device calls on one stream with set_window between them and no synchronisation: the old window entirely, then the new"""
    import torch
    N, K, S = 256, 2, 4
    w1 = ref.hann(N)
    w2 = (w1 * np.linspace(0.5, 1.5, N)).astype(np.float32)
    x = ref.make_input(ref.plan(N, K, N, S)[0], seed=21)
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, w1)
    assert blk.route().startswith("fused")
    d_x = torch.from_numpy(x).cuda()
    o1 = torch.full((S * N,), float("nan"), dtype=torch.float32, device="cuda")
    o2 = torch.full_like(o1, float("nan"))
    torch.cuda.synchronize()
    assert blk.work_device(S, [d_x], [o1]) == S * N
    blk.set_window(w2)
    assert blk.work_device(S, [d_x], [o2]) == S * N
    torch.cuda.synchronize()
    assert relerr(o1.cpu().numpy().reshape(S, N), ref.pspec(x, N, K, N, S, w1)) <= ref.TOL
    assert relerr(o2.cpu().numpy().reshape(S, N), ref.pspec(x, N, K, N, S, w2)) <= ref.TOL
    blk.stop()


def test_handle_behaviour(gpu):
    import torch
    N, K, H = 256, 6, 100
    w = ref.hann(N)
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H, scale=0.25)
    assert (blk.fft_size(), blk.navg(), blk.hop(), blk.history()) == (N, K, H, N - H)
    L_ = gpu.lib()
    assert (L_.mi355_pspec_fft_size(blk._h), L_.mi355_pspec_navg(blk._h), L_.mi355_pspec_hop(blk._h)) == (N, K, H)
    S = 4
    nin, nout = blk.plan(S)
    assert (nin, nout) == ref.plan(N, K, H, S)
    x = ref.make_input(nin)
    d_x = torch.from_numpy(x).cuda()
    for generic in (False, True):
        blk.set_generic(generic)
        blk.set_scale(0.25)
        blk.set_window(w)
        assert relerr(_run(blk, d_x, S, N), ref.pspec(x, N, K, H, S, w, scale=0.25)) <= ref.TOL
        # S = 0 is a no-op
        out = torch.full((N,), float("nan"), dtype=torch.float32, device="cuda")
        assert blk.work_device(0, [d_x[:0]], [out]) == 0
        assert L_.mi355_pspec_work_dev(blk._h, 0, None, None, None) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())
        # set_scale and set_window take effect at the next call
        blk.set_scale(3.0)
        assert relerr(_run(blk, d_x, S, N), ref.pspec(x, N, K, H, S, w, scale=3.0)) <= ref.TOL
        w2 = (w * np.linspace(0.5, 1.5, N)).astype(np.float32)
        blk.set_window(w2)
        assert relerr(_run(blk, d_x, S, N), ref.pspec(x, N, K, H, S, w2, scale=3.0)) <= ref.TOL
        blk.set_window(None)
        assert relerr(_run(blk, d_x, S, N), ref.pspec(x, N, K, H, S, None, scale=3.0)) <= ref.TOL
        # the host-pointer path gives what the device path gives
        dev = _run(blk, d_x, S, N)
        host = blk.work(x)
        assert host.shape == (S, N) and np.array_equal(host.view(np.uint32), dev.view(np.uint32))
        y = np.full(S * N, np.nan, np.float32)
        assert blk.general_work(S, [x.size], [x], [y]) == (S, S * K * H)
        assert np.array_equal(y.view(np.uint32), dev.reshape(-1).view(np.uint32))
    # short tensors are refused before the launch; in / out overlap is refused
    with pytest.raises(ValueError):
        blk.work_device(S, [d_x[:nin - 1]], [torch.empty(nout, dtype=torch.float32, device="cuda")])
    with pytest.raises(ValueError):
        blk.work_device(S, [d_x], [torch.empty(nout - 1, dtype=torch.float32, device="cuda")])
    with pytest.raises(ValueError):
        blk.general_work(S, [nin - 1], [x[:-1]], [np.empty(nout, np.float32)])
    buf = torch.zeros(nin + nout, dtype=torch.complex64, device="cuda")
    with pytest.raises(gpu.Mi355Error) as e:
        blk.work_device(S, [buf], [buf.view(torch.float32)[2 * nin - 1:]])
    assert e.value.code == -1 and "overlap" in str(e.value)
    assert blk.work_device(S, [buf], [buf.view(torch.float32)[2 * nin:]]) == nout  # the same allocation, no overlap
    with pytest.raises(gpu.Mi355Error) as e:
        gpu.clPowerSpectrum(*GPU_ARGS, N, K, w[:-1])
    assert e.value.code == -1
    with pytest.raises(gpu.Mi355Error) as e:
        gpu.clPowerSpectrum(*GPU_ARGS, 1, K)
    assert e.value.code == -3 and "fft size 1 unsupported" in str(e.value)
    blk.stop()


def test_host_path_in_pieces(gpu):
    """more input than one staged piece (64 MiB) holds: whole spectra per piece"""
    N, K, H, S = 1024, 16, 65536, 10
    x = ref.make_input(ref.plan(N, K, H, S)[0], seed=3)
    assert K * H * 8 * S > (64 << 20)
    blk = gpu.clPowerSpectrum(*GPU_ARGS, N, K, ref.hann(N), H, True)
    got = blk.work(x)
    assert got.shape == (S, N) and relerr(got, ref.pspec(x, N, K, H, S, ref.hann(N), True)) <= ref.TOL
    blk.stop()


def test_two_threads_one_handle_each(gpu):
    import torch
    N, S = 1024, 3
    cases = [(70, 512, ref.hann(N)), (5, 1024, None)]
    xs = [ref.make_input(ref.plan(N, K, H, S)[0], seed=i) for i, (K, H, _) in enumerate(cases)]
    wants = [ref.pspec(x, N, K, H, S, w) for x, (K, H, w) in zip(xs, cases)]
    blks = [gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H) for K, H, w in cases]
    d_xs = [torch.from_numpy(x).cuda() for x in xs]
    res, errs = [[], []], []

    def worker(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(20):
                    out = torch.full((S * N,), float("nan"), dtype=torch.float32, device="cuda")
                    blks[i].work_device(S, [d_xs[i]], [out])
                    st.synchronize()
                    res[i].append(out.cpu().numpy().reshape(S, N))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(res[i]) == 20 and relerr(res[i][0], wants[i]) <= ref.TOL
        assert all(np.array_equal(r.view(np.uint32), res[i][0].view(np.uint32)) for r in res[i])
    for b in blks:
        b.stop()


@pytest.mark.parametrize("generic", [False, True], ids=["fused", "generic"])
def test_one_handle_two_streams(gpu, generic):
    """the handle's workspace (fused: the partial sums of K = 2C + 3 > C frames; generic: gathered and transformed frames, H != N)
    handed between two streams: 6 calls per stream in turn with nothing waited for in between, the first of 1 spectrum and the others
    of 3, so the workspace grows after it has been used.  Every NaN-filled output is bit for bit what a second handle gives for the
    same input on one stream."""
    import torch
    N = 256
    probe = gpu.clPowerSpectrum(*GPU_ARGS, N, 1)
    C = chunk_of(probe.route())
    probe.stop()
    K, H = 2 * C + 3, N // 2 if generic else N
    w = ref.hann(N)
    blk, single = (gpu.clPowerSpectrum(*GPU_ARGS, N, K, w, H, True) for _ in range(2))
    for b in (blk, single):
        b.set_generic(generic)
        assert b.route() == ("generic N=%d batch=%d" % (N, (1 << 20) // N) if generic else "fused pow2 N=%d chunk=%d" % (N, C))
    d_xs = [torch.from_numpy(ref.make_input(ref.plan(N, K, H, 3)[0], seed=40 + s)).cuda() for s in range(2)]
    items = {S: ref.plan(N, K, H, S)[0] for S in (1, 3)}
    nan_out = lambda S: torch.full((S * N,), float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    refs = {}
    for s in range(2):
        for S in (1, 3):
            refs[s, S] = nan_out(S)
            assert single.work_device(S, [d_xs[s][:items[S]]], [refs[s, S]]) == S * N
            torch.cuda.synchronize()
            assert torch.isfinite(refs[s, S]).all()
    count = lambda k, s: 1 if (k, s) == (0, 0) else 3  # noqa: E731
    streams = [torch.cuda.Stream() for _ in range(2)]
    ys = [[nan_out(count(k, s)) for k in range(6)] for s in range(2)]
    torch.cuda.synchronize()
    for k in range(6):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                blk.work_device(count(k, s), [d_xs[s][:items[count(k, s)]]], [ys[s][k]])
    torch.cuda.synchronize()
    for s in range(2):
        for k in range(6):
            assert torch.equal(ys[s][k].view(torch.int32), refs[s, count(k, s)].view(torch.int32)), (s, k)
    for b in (blk, single):
        b.stop()
