"""GPU: clFreqXlatingFIRFilter against tests/xlate_ref.py (float64).  Every output of every case is compared, per component, with the
derived bound of the yardstick; the outputs are NaN before every call.  The yardstick takes the band-pass taps and the integer phase
from the handle (get_bandpass_taps, get_state); those are checked on their own against the closed forms.

Routes, as csrc/xlate.hip states them:
  fused    D = 2 .. 64, K <= 512, C <= 16: k_xlate, tiles of tile_out outputs (route() names it)
  generic  everything else and every handle under set_generic(True): per channel clComplexFilter + k_xl_rotate

Largest error / bound measured on an MI355X (the tests print it): fused grid 0.084 (D = 5; 0.029 ... 0.071 at the other D), generic cases
0.018 at most (1.2e-5 at K = 3000 through overlap-save, whose bound grows with K), retune 0.016 / 0.0081, skip(2^40) 0.0044 / 0.0018.
"""
import glob
import importlib.util
import os
import re
import subprocess
import threading

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import guarded
import xlate_ref as ref

pytestmark = pytest.mark.gpu
FS = 1.0e6
DS = (2, 3, 5, 8, 16, 25, 64)
KS = (1, 7, 8, 9, 65, 131)
CS = (1, 2, 3, 8)
POOL = (0.0, -250000.0, FS / 2, -FS / 2, FS / np.pi, 37.5, -123456.789, 999999.0)  # 0, negative, +-fs/2, an irrational-looking ratio
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")


def tile_of(route):
    return int(re.search(r"tile_out=(\d+)", route).group(1))


def _freqs(C, i):
    return [POOL[(i + c) % len(POOL)] for c in range(C)]


def _run(blk, d_x, n):
    """work_device on NaN-filled outputs; returns (outputs, states before the call)"""
    import torch
    C = blk.num_channels()
    states = [blk.state(c) for c in range(C)]
    outs = [torch.full((max(n, 1),), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(C)]
    assert blk.work_device(n, [d_x], outs) == n
    return [o.cpu().numpy()[:n] for o in outs], states


def _worst(blk, x, n, got, states):
    """largest error / bound over the channels, against the yardstick with the handle's own taps and integer phase"""
    D = blk.decimation()
    w = 0.0
    for c in range(blk.num_channels()):
        b = blk.bandpass_taps(c)
        want, s = ref.xlate(b, x[:ref.plan(D, b.size, n)], D, n, states[c][0], states[c][1])
        w = max(w, ref.worst(got[c], want, ref.bound(b, x[:ref.plan(D, b.size, n)], D, n, s)))
    return w


def _check_tables(blk, h, freqs):
    D = blk.decimation()
    for c, f in enumerate(freqs):
        assert ref.check_bandpass(blk.bandpass_taps(c), h, f, FS), (c, f)
        assert ref.check_inc(blk.state(c)[1], f, D, FS) and blk.state(c)[1] == ref.inc_of(f, D, FS), (c, f)
        assert blk.center_freq(c) == f


@pytest.mark.parametrize("D", DS)
def test_grid_fused(gpu, D):
    """K, C, the prototype kind, the frequencies and n_out rotate against D; n_out in {1, 2, 255, 256, 257, T - 1, T + 1, 2 T + 3}"""
    import torch
    di = DS.index(D)
    worst = 0.0
    for j in range(8):
        i = di + 7 * j
        K = KS[(i + j) % 6]
        C = CS[(i + i // 6) % 4]
        cplx = (i // 3) % 2 == 1
        h = ref.make_taps(K, cplx, seed=i)
        freqs = _freqs(C, i)
        blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, h, freqs, FS)
        T = tile_of(blk.route())
        assert blk.route() == "fused D=%d K=%d C=%d tile_out=%d" % (D, K, C, T) and T % 128 == 0
        assert (blk.history(), blk.ntaps(), blk.num_channels(), blk.decimation()) == (K, K, C, D)
        assert np.array_equal(blk.taps(), h)
        _check_tables(blk, h, freqs)
        ns = (1, 2, 255, 256, 257, T - 1, T + 1, 2 * T + 3)
        n = ns[(i + i // 5) % 8]
        x = ref.make_input(ref.plan(D, K, n), seed=i)
        assert blk.plan(n) == x.size
        got, states = _run(blk, torch.from_numpy(x).cuda(), n)
        assert all(s[0] == 0 for s in states)
        w = _worst(blk, x, n, got, states)
        worst = max(worst, w)
        assert w <= 1.0, (D, K, C, cplx, n, w)
        assert [blk.state(c)[0] for c in range(C)] == [(s[1] * n) % ref.TWO64 for s in states]
        blk.stop()
    print("D=%d worst error / bound %.3g" % (D, worst))


def test_grid_axes_are_covered():
    """the rotation of test_grid_fused visits every K, every C, both prototype kinds and every n_out class (no device needed)"""
    ks, cs, kinds, ns = set(), set(), set(), set()
    for di in range(7):
        for j in range(8):
            i = di + 7 * j
            ks.add(KS[(i + j) % 6]); cs.add(CS[(i + i // 6) % 4]); kinds.add((i // 3) % 2); ns.add((i + i // 5) % 8)
    assert ks == set(KS) and cs == set(CS) and kinds == {0, 1} and ns == set(range(8))


GENERIC = [  # D, K, C, complex, use_time, n, forced
    (1, 3000, 20, False, False, 300, False),   # D = 1, a long filter through the overlap-save path, more than 16 channels
    (1, 9, 2, True, True, 257, False),
    (100, 33, 3, False, True, 130, False),     # D above 64
    (16, 600, 2, True, False, 200, False),     # K above 512
    (8, 65, 17, False, True, 300, False),      # C above 16
    (16, 65, 3, True, True, 515, True),        # a fused shape under set_generic(True)
    (5, 131, 8, False, False, 259, True),
]


@pytest.mark.parametrize("D,K,C,cplx,use_time,n,forced", GENERIC)
def test_generic_route(gpu, D, K, C, cplx, use_time, n, forced):
    import torch
    h = ref.make_taps(K, cplx, seed=K + C)
    freqs = _freqs(C, D)
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, h, freqs, FS, use_time)
    assert blk.route().startswith("fused" if forced else "generic")
    x = ref.make_input(ref.plan(D, K, n), seed=D)
    d_x = torch.from_numpy(x).cuda()
    if forced:
        fused, st = _run(blk, d_x, n)
        assert _worst(blk, x, n, fused, st) <= 1.0
        blk.set_generic(True)
        for c in range(C):
            blk.set_phase(0, c)
    assert blk.route() == "generic D=%d K=%d C=%d" % (D, K, C)
    _check_tables(blk, h, freqs)
    got, st = _run(blk, d_x, n)
    w = _worst(blk, x, n, got, st)
    print("generic (%d, %d, %d) worst error / bound %.3g" % (D, K, C, w))
    assert w <= 1.0, w
    if forced:
        blk.set_generic(False)
        assert blk.route().startswith("fused")
        for c in range(C):
            blk.set_phase(0, c)
        again, _ = _run(blk, d_x, n)
        assert all(np.array_equal(a.view(np.uint32), f.view(np.uint32)) for a, f in zip(again, fused))
    blk.stop()


SPLITS = [  # D, K, C, complex, generic
    (5, 65, 3, True, False),    # odd D: the pieces start at both alignments
    (16, 131, 8, False, False),
    (2, 9, 2, False, False),
    (16, 65, 2, True, True),    # generic route, direct form: clComplexFilter's kernel depends on the 16-byte alignment of `in`, which
                                # an even D keeps from piece to piece
]


@pytest.mark.parametrize("D,K,C,cplx,generic", SPLITS)
def test_any_split_gives_the_same_bits(gpu, D, K, C, cplx, generic):
    """one stream as one call and cut into calls of 1, 63, 64, 65 and random sizes: bit for bit the same"""
    import torch
    rng = np.random.default_rng(D * K)
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(K, cplx, seed=3), _freqs(C, K), FS, True)
    blk.set_generic(generic)
    assert blk.route().startswith("generic" if generic else "fused")
    total = 1 + 63 + 64 + 65 + 1500
    x = ref.make_input(ref.plan(D, K, total), seed=K)
    d_x = torch.from_numpy(x).cuda()
    one, st = _run(blk, d_x, total)
    assert _worst(blk, x, total, one, st) <= 1.0
    cuts = [1, 63, 64, 65]
    while sum(cuts) < total:
        cuts.append(min(int(rng.integers(1, 700)), total - sum(cuts)))
    for c in range(C):
        blk.set_phase(0, c)
    outs = [torch.full((total,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(C)]
    done = 0
    for n in cuts:
        src = d_x[done * D:done * D + ref.plan(D, K, n)]  # in += n D
        assert blk.work_device(n, [src], [o[done:done + n] for o in outs]) == n
        done += n
    for c in range(C):
        assert np.array_equal(outs[c].cpu().numpy().view(np.uint32), one[c].view(np.uint32)), c
    assert [blk.state(c) for c in range(C)] == [((s[1] * total) % ref.TWO64, s[1]) for s in st]
    blk.stop()


BOUNDS = [  # D, K, C, complex, generic, n
    (16, 65, 3, False, False, 300),
    (3, 9, 2, True, False, 1025),     # odd D
    (64, 131, 8, False, False, 130),
    (2, 1, 1, False, False, 257),
    (16, 65, 2, True, True, 300),     # a fused shape forced generic
    (1, 40, 2, False, True, 500),     # generic by shape
]


@pytest.mark.parametrize("D,K,C,cplx,generic,n", BOUNDS)
def test_guard_bands_and_alignment(gpu, D, K, C, cplx, generic, n):
    """the input holds exactly n D + K - 1 items with NaN on both sides, every output exactly n items between sentinels; `in` and every
    output at 0 and at 8 bytes past a 16-byte boundary.  Fused route: the same bits at both alignments."""
    import torch
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(K, cplx, seed=5), _freqs(C, 2), FS, True)
    blk.set_generic(generic)
    assert blk.route().startswith("generic" if generic else "fused")
    x = ref.make_input(ref.plan(D, K, n), seed=n)
    res = []
    for off_in, off_out in ((0, 0), (1, 1), (1, 0), (0, 1)):
        wi, vi = guarded.guarded_input(x, guarded.pad_items(8), off_in, device="cuda")
        outs = [guarded.guarded_output(n, np.complex64, guarded.pad_items(8), off_out, device="cuda") for _ in range(C)]
        assert vi.data_ptr() % 16 == 8 * off_in and all(v.data_ptr() % 16 == 8 * off_out for _, v in outs)
        for c in range(C):
            blk.set_phase(0, c)
        st = [blk.state(c) for c in range(C)]
        assert blk.work_device(n, [vi], [v for _, v in outs]) == n
        torch.cuda.synchronize()
        guarded.check_guards(wi, vi, "input")
        for c, (w, v) in enumerate(outs):
            guarded.check_guards(w, v, "output %d" % c)
        got = [guarded.to_numpy(v) for _, v in outs]
        assert _worst(blk, x, n, got, st) <= 1.0, (off_in, off_out)
        res.append(got)
    if not generic:
        for r in res[1:]:
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r, res[0]))
    blk.stop()


def test_misaligned_and_null_pointers_are_refused(gpu):
    import ctypes as C
    import torch
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, 4, np.ones(9, np.float32), [1000.0, 2000.0], FS)
    L_ = gpu.lib()
    x = torch.from_numpy(ref.make_input(104)).cuda()
    outs = [torch.full((24,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(2)]

    def call(din, dout0, dout1):
        ptrs = (C.c_void_p * 2)(outs[0].data_ptr() + dout0 if dout0 is not None else None, outs[1].data_ptr() + dout1)
        return L_.mi355_xlate_work_dev(blk._h, 16, x.data_ptr() + din, ptrs, None)

    for args in ((4, 0, 0), (0, 4, 0), (0, 0, 12), (0, None, 0)):
        assert call(*args) == -1, args
    assert L_.mi355_xlate_work_dev(blk._h, 16, None, None, None) == -1
    assert blk.state(0)[0] == 0 and blk.state(1)[0] == 0  # nothing ran, nothing advanced
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(torch.view_as_real(o)).all()) for o in outs)
    assert L_.mi355_xlate_work_dev(blk._h, 0, None, None, None) == 0  # no output: a no-op
    with pytest.raises(gpu.Mi355Error) as e:  # in and an output overlap
        blk.work_device(16, [x], [x[60:], outs[1]])
    assert e.value.code == -1 and "overlap" in str(e.value)
    with pytest.raises(ValueError):
        blk.work_device(16, [x[:4 * 16 + 7]], outs)  # one item short of 16 * 4 + 9 - 1
    with pytest.raises(ValueError):
        blk.work_device(16, [x], [outs[0]])
    for c, f in ((2, 1.0), (-1, 1.0), (0, float("nan")), (0, float("inf"))):
        with pytest.raises(gpu.Mi355Error) as e:
            blk.set_center_freq(f, c)
        assert e.value.code == -1
    assert blk.center_freq(0) == 1000.0
    blk.stop()


def test_retune_keeps_the_phase(gpu):
    """a tone through a boxcar, the centre frequency changed between two calls: both halves match the yardstick with the carried phase,
    P is the same integer before and after set_center_freq, and |y| does not jump (the tone stays well inside the main lobe: the
    boxcar's gain at 1 kHz and at 2 kHz from its centre differs by 0.2 %)"""
    import torch
    D, K, n = 8, 16, 400
    ft, f1, f2 = 100000.0, 101000.0, 98000.0
    t = np.arange(ref.plan(D, K, 2 * n)) - (K - 1)
    x = np.exp(2j * np.pi * ft / FS * t).astype(np.complex64)
    for generic in (False, True):
        blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, np.full(K, 1.0 / K, np.float32), f1, FS, True)
        blk.set_generic(generic)
        d_x = torch.from_numpy(x).cuda()
        a, st_a = _run(blk, d_x[:ref.plan(D, K, n)], n)
        assert _worst(blk, x, n, a, st_a) <= 1.0
        before = blk.state(0)
        blk.set_center_freq(f2)
        after = blk.state(0)
        assert after[0] == before[0] == (st_a[0][1] * n) % ref.TWO64 and after[1] == ref.inc_of(f2, D, FS) != before[1]
        assert ref.check_bandpass(blk.bandpass_taps(0), np.full(K, 1.0 / K, np.float32), f2, FS)
        x2 = x[n * D:]
        b, st_b = _run(blk, d_x[n * D:], n)
        assert st_b[0] == after
        w = _worst(blk, x2, n, b, st_b)
        print("retune (generic=%s) worst error / bound %.3g" % (generic, w))
        assert w <= 1.0
        mag = np.abs(np.concatenate([a[0], b[0]]))
        assert np.abs(np.diff(mag)).max() <= 0.005 and abs(mag[n] - mag[n - 1]) <= 0.005 and mag.min() >= 0.99
        # the phase of the output does not jump either: one output step at 2 kHz offset turns it by 2 pi 2000 D / fs = 0.1 rad, the
        # boxcar's own phase moves by pi (K - 1) 3000 / fs = 0.14 rad
        step = np.angle(b[0][0] * np.conj(a[0][-1]))
        assert abs(step) <= 0.3, step
        blk.stop()


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("setter", ["set_taps", "set_center_freq"])
def test_setter_between_enqueued_calls(gpu, setter, generic):
    """two work_device calls on one stream with a setter between them and no synchronisation: the old table entirely, then the new.
    The yardstick's taps and phases are read from the handle before each call."""
    import torch
    D, K, C, n = 4, 33, 2, 1000
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(K, False, seed=3), [250000.0, -37.5], FS)
    assert blk.route().startswith("fused")
    blk.set_generic(generic)
    assert blk.route().startswith("generic" if generic else "fused")
    x = ref.make_input(ref.plan(D, K, 2 * n), seed=9)
    d_x = torch.from_numpy(x).cuda()
    outs = [[torch.full((n,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(C)] for _ in range(2)]
    torch.cuda.synchronize()
    seen = []
    for call in range(2):
        if call == 1:
            if setter == "set_taps":
                blk.set_taps(ref.make_taps(K, False, seed=4))
            else:
                blk.set_center_freq(-123456.789, 1)
        seen.append(([blk.bandpass_taps(c) for c in range(C)], [blk.state(c) for c in range(C)]))
        assert blk.work_device(n, [d_x[call * n * D:]], outs[call]) == n
    torch.cuda.synchronize()
    assert not np.array_equal(seen[0][0][1], seen[1][0][1])
    for call, (bs, states) in enumerate(seen):
        xin = x[call * n * D:][:ref.plan(D, K, n)]
        for c in range(C):
            want, s = ref.xlate(bs[c], xin, D, n, states[c][0], states[c][1])
            w = ref.worst(outs[call][c].cpu().numpy(), want, ref.bound(bs[c], xin, D, n, s))
            assert w <= 1.0, (call, c, w)
    blk.stop()


def test_skip_is_exact_far_into_a_stream(gpu):
    """skip(2^40), then a call: the phase is inc 2^40 mod 2^64 exactly (a float or double accumulator is not), and the outputs match the
    yardstick at that index"""
    import torch
    D, K, C, n = 16, 65, 3, 300
    freqs = [FS / np.pi, -123456.789, 37.5]
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(K, False, seed=1), freqs, FS)
    x = ref.make_input(ref.plan(D, K, n), seed=40)
    d_x = torch.from_numpy(x).cuda()
    for generic in (False, True):
        blk.set_generic(generic)
        for c in range(C):
            blk.set_phase(0, c)
        blk.skip(1 << 40)
        for c in range(C):
            assert blk.state(c) == ((ref.inc_of(freqs[c], D, FS) << 40) % ref.TWO64, ref.inc_of(freqs[c], D, FS))
        got, st = _run(blk, d_x, n)
        w = _worst(blk, x, n, got, st)
        print("skip (generic=%s) worst error / bound %.3g" % (generic, w))
        assert w <= 1.0
        # the same outputs come from the phase set directly
        for c in range(C):
            blk.set_phase(st[c][0], c)
        again, _ = _run(blk, d_x, n)
        assert all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(again, got))
    with pytest.raises(gpu.Mi355Error):
        blk.skip(-1)
    blk.stop()


def test_set_taps_keeps_the_phase_and_picks_the_route_again(gpu):
    import torch
    D, C, n = 8, 2, 200
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(33, True, seed=2), [250000.0, -37.5], FS, True)
    x = ref.make_input(ref.plan(D, 700, n), seed=8)
    d_x = torch.from_numpy(x).cuda()
    _run(blk, d_x, n)
    p = [blk.state(c) for c in range(C)]
    for K, route in ((9, "fused"), (700, "generic"), (65, "fused")):
        h = ref.make_taps(K, True, seed=K)
        blk.set_taps(h)
        assert blk.route().startswith(route) and blk.ntaps() == K and np.array_equal(blk.taps(), h)
        assert [blk.state(c) for c in range(C)] == p
        got, st = _run(blk, d_x, n)
        assert _worst(blk, x, n, got, st) <= 1.0, K
        p = [blk.state(c) for c in range(C)]
    with pytest.raises(TypeError):
        gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, np.ones(4, np.float32), 0.0, FS).set_taps(np.ones(4, np.complex64))
    blk.stop()


def test_host_path_gives_the_device_path_bits(gpu):
    """work() on host pointers: a scheduler-sized call, and one of more than one staged piece (3 MiB of input: three pieces)"""
    import torch
    for D, K, C, n, generic in ((16, 65, 2, 512, False), (16, 65, 2, 24576, False), (4, 33, 3, 1000, True)):
        blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(K, True, seed=6), _freqs(C, 4), FS, True)
        blk.set_generic(generic)
        x = ref.make_input(ref.plan(D, K, n), seed=n)
        dev, st = _run(blk, torch.from_numpy(x).cuda(), n)
        for c in range(C):
            blk.set_phase(0, c)
        ys = [np.full(n, complex(np.nan, np.nan), np.complex64) for _ in range(C)]
        assert blk.work(n, [x], ys) == n
        assert all(np.array_equal(y.view(np.uint32), d.view(np.uint32)) for y, d in zip(ys, dev))
        assert [blk.state(c)[0] for c in range(C)] == [(s[1] * n) % ref.TWO64 for s in st]
        with pytest.raises(ValueError):
            blk.work(n, [x[:-1]], ys)
        blk.stop()


def test_two_tones_land_at_dc_of_their_own_outputs(gpu):
    """end to end: one capture with two tones, C = 2, a 32-tap boxcar whose nulls hold the other tone"""
    import torch
    D, K, n = 8, 32, 600
    f0, f1 = FS / 8, -FS / 4
    t = np.arange(ref.plan(D, K, n)) - (K - 1)
    x = (np.exp(2j * np.pi * f0 / FS * t) + 0.5 * np.exp(2j * np.pi * f1 / FS * t)).astype(np.complex64)
    blk = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, np.full(K, 1.0 / K, np.float32), [f0, f1], FS)
    got, _ = _run(blk, torch.from_numpy(x).cuda(), n)
    assert np.abs(got[0] - 1.0).max() <= 1e-5 and np.abs(got[1] - 0.5).max() <= 1e-5
    spec = np.abs(np.fft.fft(got[0][:512]))
    assert spec.argmax() == 0 and np.sort(spec)[-2] <= 1e-4 * spec[0]
    blk.stop()


def test_two_threads_one_handle_each(gpu):
    import torch
    cases = [(16, 65, 3, False), (5, 33, 2, True)]
    n = 700
    blks = [gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, ref.make_taps(K, cplx, seed=K), _freqs(C, K), FS) for D, K, C, cplx in cases]
    xs = [ref.make_input(ref.plan(D, K, n), seed=D) for D, K, C, _ in cases]
    d_xs = [torch.from_numpy(x).cuda() for x in xs]
    res, errs = [[], []], []

    def worker(i):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(20):
                    for c in range(cases[i][2]):
                        blks[i].set_phase(0, c)
                    outs = [torch.full((n,), complex(np.nan, np.nan), dtype=torch.complex64, device="cuda") for _ in range(cases[i][2])]
                    blks[i].work_device(n, [d_xs[i]], outs)
                    st.synchronize()
                    res[i].append([o.cpu().numpy() for o in outs])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(2):
        C = cases[i][2]
        states = [(0, blks[i].state(c)[1]) for c in range(C)]
        assert len(res[i]) == 20 and _worst(blks[i], xs[i], n, res[i][0], states) <= 1.0
        assert all(np.array_equal(r[c].view(np.uint32), res[i][0][c].view(np.uint32)) for r in res[i] for c in range(C))
    for b in blks:
        b.stop()


def test_info_line_names_the_route(gpu):
    got = []
    gpu.set_log_callback(lambda level, msg: got.append((level, msg)))
    try:
        gpu.clFreqXlatingFIRFilter(*GPU_ARGS[:3], 0, 16, np.ones(65, np.float32), [0.0, 1.0], FS, False, 1).stop()
        gpu.clFreqXlatingFIRFilter(*GPU_ARGS[:3], 0, 1, np.ones(9, np.float32), 0.0, FS, True, 1).stop()
    finally:
        gpu.set_log_callback(None)
    text = [m for lvl, m in got if lvl == 1 and m.startswith("clFreqXlatingFIRFilter")]
    assert any("decimation 16, 65 real taps, 2 channels: fused D=16 K=65 C=2 tile_out=" in m and "k_xlate" in m for m in text), text
    assert any("decimation 1, 9 real taps, 1 channel: generic D=1 K=9 C=1" in m for m in text), text


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, two calls chained, the freq port, set_taps' empty call"""
    mod = _pybind()
    D, K, n = 8, 33, 300
    h = ref.make_taps(K, False, seed=11)
    freqs = [250000.0, -123456.789]
    blk = mod.clFreqXlatingFIRFilter(*GPU_ARGS, D, h.tolist(), freqs, FS)
    assert (blk.num_channels(), blk.history(), blk.decimation()) == (2, K, D) and blk.route().startswith("fused")
    assert np.array_equal(np.array(blk.taps()), h.astype(np.complex64))
    x = ref.make_input(ref.plan(D, K, 2 * n), seed=12)
    py = gpu.clFreqXlatingFIRFilter(*GPU_ARGS, D, h, freqs, FS)  # the ctypes class: the same library underneath
    ys = [np.full(2 * n, complex(np.nan, np.nan), np.complex64) for _ in range(2)]
    want = [np.empty(2 * n, np.complex64) for _ in range(2)]
    for k in range(2):
        seg = x[k * n * D:k * n * D + ref.plan(D, K, n)]
        assert blk.work(n, [seg], [y[k * n:(k + 1) * n] for y in ys]) == n
        py.work(n, [seg], [w[k * n:(k + 1) * n] for w in want])
    states = [(0, ref.inc_of(f, D, FS)) for f in freqs]
    assert _worst(py, x, 2 * n, ys, states) <= 1.0
    assert all(np.array_equal(y.view(np.uint32), w.view(np.uint32)) for y, w in zip(ys, want))
    with pytest.raises(ValueError):
        blk.work(n, [x[:ref.plan(D, K, n) - 1]], [y[:n] for y in ys])
    assert blk.post_freq(1234.5) and blk.center_freq(0) == 1234.5 and blk.center_freq(1) == freqs[1]
    blk.set_taps([1.0 + 0j] * 5)
    assert blk.history() == K and blk.work(n, [x], [y[:n] for y in ys]) == 0 and blk.history() == 5
    blk.set_generic(True)
    assert blk.route().startswith("generic") and blk.work(10, [x], [y[:10] for y in ys]) == 10
    with pytest.raises(ValueError):
        mod.clFreqXlatingFIRFilter(*GPU_ARGS, D, h.tolist(), [], FS)
    py.stop()


def test_cli_xlate_only(gpu):
    r = subprocess.run([CLI, "--xlate-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(rows) == 3 and all(l.startswith("clFreqXlatingFIRFilter") and l.rstrip().endswith("ok") for l in rows), r.stdout
