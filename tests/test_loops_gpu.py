"""clSignalSource and clCostasLoop on the device against the float64 restatement (tests/loops_ref.py): single calls, consecutive
calls, chunking, streams, guard bands, host calls of more than one piece, short tensors, a source -> multiply -> loop chain, the pybind blocks and the CLI.

Tolerances (derived, not fitted):
  signal source, complex / float   |got - ref| <= 2^-22 |A|: the result is the float rounding of a double (half a float ulp at
                                   magnitude A, 2^-24 A); the double is off by at most half an ulp of an argument below 2^22 rad
                                   (< 5e-10) plus a few 1e-16.  Four times the rounding.
  signal source, int               equal, except where the restatement lies within 1e-6 of an integer (test_loops.py caps those)
  Costas                           |got - ref| <= 1e-5 max|in| (the project's float parity bar); test_loops.py proves that every
                                   case here moves by less than a tenth of that under 1e-9 relative trig noise
  Costas state (double)            rel 1e-9"""
import os
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import guarded
import loops_ref as ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
COSTAS_TOL = 1e-5
STATE_RTOL = 1e-9
SIG_TOL = 2.0 ** -22


def _close_state(got, want):
    for g, w in zip(got, want):
        assert np.all(np.abs(np.asarray(g) - np.asarray(w)) <= STATE_RTOL * np.maximum(1.0, np.abs(w))), (g, w)


# ---------------------------------------------------------------------------------------------------------- signal source
KINDS = {"complex": (1, 1, np.complex64), "float-cos": (2, 1, np.float32), "float-sin": (2, 2, np.float32)}


def _source(gpu, dtype, wave, ratio, amp):
    return gpu.clSignalSource(dtype, *GPU_ARGS, ref.SIG_SAMP_RATE, wave, ratio * ref.SIG_SAMP_RATE, amp)


def _gen(blk, n, npdt):
    import torch
    out = torch.full((n,), float("nan") if npdt != np.int32 else 0x5A5A5A5A, dtype=guarded._TORCH_OF[np.dtype(npdt)], device="cuda")
    assert blk.work_device(n, [], [out]) == n
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_sig(got, want, amp):
    if np.iscomplexobj(want):  # per component
        err = max(np.abs(got.real.astype(np.float64) - want.real).max(), np.abs(got.imag.astype(np.float64) - want.imag).max())
    else:
        err = np.abs(got.astype(np.float64) - want).max()
    assert err <= SIG_TOL * abs(amp), (err, SIG_TOL * abs(amp))


@pytest.mark.parametrize("amp", ref.SIG_AMPS)
@pytest.mark.parametrize("ratio", ref.SIG_RATIOS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_signal_source_single_calls(gpu, kind, ratio, amp):
    dtype, wave, npdt = KINDS[kind]
    inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    for n in ref.SIG_N:
        blk = _source(gpu, dtype, wave, ratio, amp)
        pos0, rate = blk.get_state()
        assert pos0 == 0.0 and rate == inc
        want, pos = ref.sig_call(0.0, inc, n, amp, kind.split("-")[0], wave)
        _check_sig(_gen(blk, n, npdt), want, amp)
        assert blk.get_state()[0] == pos, n   # the host-side advance and wrap, bit for bit
        assert blk._L.mi355_sigsource_work_dev(blk._h, 0, None, None) == 0 and blk.get_state()[0] == pos   # n = 0: a successful no-op


def _check_int(got, want):
    skip = ref.near_integer(want)
    assert skip.sum() <= ref.INT_CAP * len(want)
    assert np.array_equal(got[~skip], np.trunc(want[~skip]).astype(np.int32))


@pytest.mark.parametrize("ratio,amp,wave", ref.SIG_INT_CASES)
def test_signal_source_int_truncates_the_double(gpu, ratio, amp, wave):
    inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    for n in ref.SIG_N:
        blk = _source(gpu, 3, wave, ratio, amp)
        blk.set_phase(ref.SIG_INT_PHASE)
        want, pos = ref.sig_call(ref.SIG_INT_PHASE, inc, n, amp, "int", wave)
        _check_int(_gen(blk, n, np.int32), want)
        assert blk.get_state()[0] == pos
    blk = _source(gpu, 3, wave, ratio, amp)   # consecutive ragged calls as one stream
    blk.set_phase(ref.SIG_INT_PHASE)
    pos, got, want = ref.SIG_INT_PHASE, [], []
    for n in ref.SIG_RAGGED:
        v, pos = ref.sig_call(pos, inc, n, amp, "int", wave)
        want.append(v)
        got.append(_gen(blk, n, np.int32))
    _check_int(np.concatenate(got), np.concatenate(want))


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_signal_source_consecutive_calls_setters_and_host_path(gpu, kind):
    dtype, wave, npdt = KINDS[kind]
    ratio, amp = -0.37, 1000.5
    inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    blk = _source(gpu, dtype, wave, ratio, amp)
    pos = 0.0
    for n in ref.SIG_RAGGED:   # every call continues where the last one stopped, through the wrap
        want, pos = ref.sig_call(pos, inc, n, amp, kind.split("-")[0], wave)
        _check_sig(_gen(blk, n, npdt), want, amp)
        assert blk.get_state()[0] == pos
    blk.set_frequency(0.01234 * ref.SIG_SAMP_RATE)   # keeps the phase
    inc2 = ref.sig_inc(0.01234 * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    assert blk.get_state() == (pos, inc2)
    want, pos = ref.sig_call(pos, inc2, 777, amp, kind.split("-")[0], wave)
    _check_sig(_gen(blk, 777, npdt), want, amp)
    blk.set_phase(1.25)
    assert blk.get_state() == (1.25, inc2)
    n = 70000   # the host path, blocking
    want, pos = ref.sig_call(1.25, inc2, n, amp, kind.split("-")[0], wave)
    host = np.empty(n, npdt)
    assert blk.work(n, [], [host]) == n
    _check_sig(host, want, amp)
    assert blk.get_state()[0] == pos


HOST_PIECE = 1 << 21   # items of a piece of either block's host path, over all streams (csrc/loops.hip kHostChunkItems)


@pytest.mark.parametrize("kind", ["complex", "float-sin"])
def test_signal_source_host_path_in_two_pieces(gpu, kind):
    """work(2^21 + 5): one full piece and one of five items, whose first item is item 2^21 of the call.  The bits of one
    work_device call from the same phase, the same state afterwards, and the restatement.  (The frequency keeps the largest
    argument, 1.6e5 rad, below the 2^22 rad of the tolerance's derivation.)"""
    dtype, wave, npdt = KINDS[kind]
    ratio, amp, n = 0.01234, 1000.5, HOST_PIECE + 5
    inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    dev, blk = _source(gpu, dtype, wave, ratio, amp), _source(gpu, dtype, wave, ratio, amp)
    dev.set_phase(1.25)
    blk.set_phase(1.25)
    one = _gen(dev, n, npdt)
    host = np.full(n, np.nan, npdt)
    assert blk.work(n, [], [host]) == n
    assert np.array_equal(host.view(np.uint32), one.view(np.uint32))
    assert blk.get_state() == dev.get_state()
    want, pos = ref.sig_call(1.25, inc, n, amp, kind.split("-")[0], wave)
    _check_sig(host, want, amp)
    assert blk.get_state() == (pos, inc)


@pytest.mark.parametrize("kind,offset", [("complex", 0), ("complex", 1), ("float-sin", 0), ("float-sin", 1), ("float-sin", 3),
                                         ("int-cos", 0), ("int-cos", 2)])
def test_signal_source_guard_bands(gpu, kind, offset):
    """n = 4099 at every alignment of the output (16-byte vector stores with a scalar head and tail): nothing outside is written,
    every item inside is"""
    import torch
    dtype, wave, npdt = {"int-cos": (3, 1, np.int32)}.get(kind) or KINDS[kind]
    n, ratio, amp = 4099, 0.01234, 1000.5
    inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    blk = _source(gpu, dtype, wave, ratio, amp)
    blk.set_phase(ref.SIG_INT_PHASE)
    whole, view = guarded.guarded_output(n, npdt, guarded.pad_items(np.dtype(npdt).itemsize, 4096), offset, device="cuda")
    blk.work_device(n, [], [view])
    torch.cuda.synchronize()
    guarded.check_guards(whole, view, "signal source output")
    want, _ = ref.sig_call(ref.SIG_INT_PHASE, inc, n, amp, kind.split("-")[0], wave)
    if npdt == np.int32:
        _check_int(guarded.to_numpy(view), want)
    else:
        _check_sig(guarded.to_numpy(view), want, amp)


# ---------------------------------------------------------------------------------------------------------- Costas loop
def _loop(gpu, order, streams):
    return gpu.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, order, 0, streams)


def _run_loop(blk, x, nitems, sizes=None, stream=None, want_freq=True):
    """x on the device through work_device in calls of `sizes` items (default: one call) -> (out, freq_out) on the host"""
    import torch
    S = blk.num_streams
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.full((nitems * S,), float("nan"), dtype=torch.complex64, device="cuda")
    d_f = torch.full((nitems * S,), float("nan"), dtype=torch.float32, device="cuda") if want_freq else None
    torch.cuda.synchronize()
    at = 0
    for m in sizes or (nitems,):
        a, b = at * S, (at + m) * S
        outs = [d_out[a:b], d_f[a:b]] if want_freq else [d_out[a:b]]
        if stream is not None:
            with torch.cuda.stream(stream):
                blk.work_device(m, [d_in[a:b]], outs)
        else:
            blk.work_device(m, [d_in[a:b]], outs)
        at += m
    assert at == nitems
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), (d_f.cpu().numpy() if want_freq else None)


def _check_costas(got, got_f, want, want_f, x):
    scale = float(np.abs(x).max())
    err = max(np.abs(got.real.astype(np.float64) - want.real).max(), np.abs(got.imag.astype(np.float64) - want.imag).max())
    assert err <= COSTAS_TOL * scale, (err, COSTAS_TOL * scale)
    if got_f is not None:
        assert np.abs(got_f.astype(np.float64) - want_f).max() <= COSTAS_TOL


@pytest.mark.parametrize("nitems", ref.COSTAS_NITEMS)
@pytest.mark.parametrize("streams", ref.COSTAS_STREAMS)
@pytest.mark.parametrize("order", ref.COSTAS_ORDERS)
def test_costas_shape_grid(gpu, order, streams, nitems):
    x, _ = ref.costas_input(order, streams, nitems)
    want, want_f, want_state = ref.costas_expected(order, streams, nitems)
    blk = _loop(gpu, order, streams)
    _close_state(blk.get_state(), (np.zeros(streams),) * 3)
    got, got_f = _run_loop(blk, x, nitems)
    _check_costas(got, got_f, want, want_f, x)
    _close_state(blk.get_state(), want_state)
    assert blk._L.mi355_costas_work_dev(blk._h, 0, None, None, None, None) == 0   # nitems = 0: a successful no-op, the state stays
    _close_state(blk.get_state(), want_state)


def test_costas_long_single_stream_locks(gpu):
    """2^18 items of one stream: drift over many wraps of the phase, and the point of the block -- the loop has found the offset"""
    order, n = ref.COSTAS_LONG
    x, off = ref.costas_long_input()
    want, want_f, want_state = ref.costas_long_expected()
    blk = _loop(gpu, order, 1)
    got, got_f = _run_loop(blk, x, n)
    _check_costas(got, got_f, want, want_f, x)
    state = blk.get_state()
    _close_state(state, want_state)
    assert abs(state[1][0] - off[0]) <= 0.1 * abs(off[0])
    assert blk.get_frequency() == state[1][0] and blk.get_phase() == state[0][0]


@pytest.mark.parametrize("streams", [1, 100])
@pytest.mark.parametrize("order", ref.COSTAS_ORDERS)
def test_costas_chunks_repeats_and_streams_are_bit_identical(gpu, order, streams):
    import torch
    n = 4097
    x, _ = ref.costas_input(order, streams, n)
    blk = _loop(gpu, order, streams)
    one, one_f = _run_loop(blk, x, n)
    state = blk.get_state()
    runs = [dict(sizes=(1, 63, 500, n - 564)), dict(), dict(stream=torch.cuda.Stream()),
            dict(sizes=(1, 63, 500, n - 564), stream=torch.cuda.Stream()), dict(want_freq=False)]
    for kw in runs:
        blk.set_state(0.0, 0.0)
        got, got_f = _run_loop(blk, x, n, **kw)
        assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), kw
        if got_f is not None:
            assert np.array_equal(got_f.view(np.uint32), one_f.view(np.uint32)), kw
        for a, b in zip(blk.get_state(), state):
            assert np.array_equal(a, b), kw
    # a call on the default stream and the next on a side stream, with no synchronisation in between: the handle orders them
    blk.set_state(0.0, 0.0)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.empty(n * streams, dtype=torch.complex64, device="cuda")
    side = torch.cuda.Stream()
    half = 2000 * streams
    blk.work_device(2000, [d_in[:half]], [d_out[:half]])
    with torch.cuda.stream(side):
        blk.work_device(n - 2000, [d_in[half:]], [d_out[half:]])
    for a, b in zip(blk.get_state(), state):   # (waits for the handle's last call)
        assert np.array_equal(a, b)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), one.view(np.uint32))
    # the host path: the same bits again
    blk.set_state(0.0, 0.0)
    host, host_f = np.empty(n * streams, np.complex64), np.empty(n * streams, np.float32)
    assert blk.work(n, [x], [host, host_f]) == n
    assert np.array_equal(host.view(np.uint32), one.view(np.uint32)) and np.array_equal(host_f.view(np.uint32), one_f.view(np.uint32))


def test_costas_host_path_in_three_pieces(gpu):
    """64 streams, 2 * 32768 + 3 items each: the host path runs two pieces of 2^21 / 64 items per stream and one of three.  With the
    frequency output: output, frequency output and final state are the bits of ONE work_device call, and the whole array is held to
    the restatement (2.8 s of CPU, once)."""
    order, streams, n = ref.COSTAS_PIECES
    assert (HOST_PIECE // streams) * 2 + 3 == n
    x, _ = ref.costas_pieces_input()
    dev = _loop(gpu, order, streams)
    one, one_f = _run_loop(dev, x, n)
    blk = _loop(gpu, order, streams)
    host, host_f = np.full(n * streams, np.nan, np.complex64), np.full(n * streams, np.nan, np.float32)
    assert blk.work(n, [x], [host, host_f]) == n
    assert np.array_equal(host.view(np.uint32), one.view(np.uint32)) and np.array_equal(host_f.view(np.uint32), one_f.view(np.uint32))
    state = blk.get_state()
    for a, b in zip(state, dev.get_state()):
        assert np.array_equal(a, b)
    want, want_f, want_state = ref.costas_pieces_expected()
    _check_costas(host, host_f, want, want_f, x)
    _close_state(state, want_state)


@pytest.mark.parametrize("order", ref.COSTAS_ORDERS)
def test_costas_stream_zero_of_many_equals_the_single_stream_kernel(gpu, order):
    n, streams = 4097, 100
    x, _ = ref.costas_input(order, streams, n)
    many, many_f = _run_loop(_loop(gpu, order, streams), x, n)
    x0 = np.ascontiguousarray(x.reshape(n, streams)[:, 0])
    single, single_f = _run_loop(_loop(gpu, order, 1), x0, n)
    m0, f0 = many.reshape(n, streams)[:, 0], many_f.reshape(n, streams)[:, 0]
    assert np.abs(m0 - single).max() <= COSTAS_TOL * float(np.abs(x0).max())   # different kernels: not bitwise
    assert np.abs(f0 - single_f).max() <= COSTAS_TOL


def test_costas_setters(gpu):
    order, streams, n, start = ref.COSTAS_START
    x, _ = ref.costas_input(order, streams, n)
    blk = _loop(gpu, order, streams)
    assert (blk.get_alpha(), blk.get_beta()) == ref.costas_gains(ref.LOOP_BW) and blk.get_loop_bandwidth() == ref.LOOP_BW
    blk.set_state(start[0], start[1])
    _close_state(blk.get_state()[:2], start[:2])
    blk.set_phase(start[0])   # None leaves the other part as it is
    _close_state(blk.get_state()[:2], start[:2])
    want, want_f, want_state = ref.costas(x, order, ref.LOOP_BW, streams, state=start)
    got, got_f = _run_loop(blk, x, n)
    _check_costas(got, got_f, want, want_f, x)
    _close_state(blk.get_state(), want_state)
    blk.set_loop_bandwidth(0.02)
    assert (blk.get_alpha(), blk.get_beta()) == ref.costas_gains(0.02)
    with pytest.raises(gpu.Mi355Error):
        blk.set_loop_bandwidth(-1.0)
    with pytest.raises(gpu.Mi355Error):
        gpu.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, 2, 0, 4097)   # more streams than supported


@pytest.mark.parametrize("streams,nitems,offset", [(65, 65, 0), (65, 65, 1), (1, 65, 1), (1, 4097, 0)])
def test_costas_guard_bands(gpu, streams, nitems, offset):
    """NaN around the input, sentinels around both outputs, at 16-byte and at 8-byte alignment: a partial last wave (65 streams), a
    partial last tile and the look-ahead loads stay inside"""
    import torch
    order = 4
    x, _ = ref.costas_input(order, streams, nitems)
    want, want_f, _ = ref.costas_expected(order, streams, nitems)
    n = nitems * streams
    pad = guarded.pad_items(8, 64 * streams)
    wi, vi = guarded.guarded_input(x, pad, offset, device="cuda")
    wo, vo = guarded.guarded_output(n, np.complex64, pad, offset, device="cuda")
    wf, vf = guarded.guarded_output(n, np.float32, guarded.pad_items(4, 64 * streams), offset, device="cuda")
    blk = _loop(gpu, order, streams)
    blk.work_device(nitems, [vi], [vo, vf])
    torch.cuda.synchronize()
    for w, v, name in ((wi, vi, "input"), (wo, vo, "output"), (wf, vf, "frequency output")):
        guarded.check_guards(w, v, name)
    _check_costas(guarded.to_numpy(vo), guarded.to_numpy(vf), want, want_f, x)


def test_work_device_refuses_short_tensors(gpu):
    import torch
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
    src = gpu.clSignalSource(1, *GPU_ARGS, 48000.0, 1, 1000.0, 1.0)
    with pytest.raises(ValueError):
        src.work_device(100, [], [z(199)])
    assert src.work_device(100, [], [z(200)]) == 100
    srci = gpu.clSignalSource(3, *GPU_ARGS, 48000.0, 2, 1000.0, 100.0)
    with pytest.raises(ValueError):
        srci.work_device(100, [], [z(99, torch.int32)])
    loop = gpu.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, 2, 0, 3)
    with pytest.raises(ValueError):
        loop.work_device(100, [z(2 * 300 - 2)], [z(2 * 300)])
    with pytest.raises(ValueError):
        loop.work_device(100, [z(2 * 300)], [z(2 * 300 - 2)])
    with pytest.raises(ValueError):
        loop.work_device(100, [z(2 * 300)], [z(2 * 300), z(299)])
    assert loop.work_device(100, [z(2 * 300)], [z(2 * 300), z(300)]) == 100
    with pytest.raises(ValueError):
        loop.work(100, [np.zeros(299, np.complex64)], [np.zeros(300, np.complex64)])
    torch.cuda.synchronize()


def test_chain_source_multiply_loop_on_the_device(gpu):
    """clSignalSource -> clMathOp multiply turns a QPSK stream by a known offset; clCostasLoop takes it out again.  The QPSK set is
    its own image under the loop's 90-degree ambiguity, so every settled output sits near one of its four points."""
    import torch
    n, offset = 8192, 0.02   # rad / item
    rng = np.random.default_rng(21)
    sym = rng.integers(0, 4, n)
    qpsk = (np.exp(1j * (np.pi / 2 * sym + np.pi / 4)) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    src = gpu.clSignalSource(gpu.DTYPE_COMPLEX, *GPU_ARGS, 1.0, 1, offset / ref.TWO_PI, 1.0)
    mul = gpu.clMathOp(gpu.DTYPE_COMPLEX, *GPU_ARGS, gpu.MATHOP_MULTIPLY)
    loop = gpu.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, 4)
    d_sym = torch.from_numpy(qpsk).cuda()
    tone, mixed, out = (torch.empty(n, dtype=torch.complex64, device="cuda") for _ in range(3))
    src.work_device(n, [], [tone])
    mul.work_device(n, [d_sym, tone], [mixed])
    loop.work_device(n, [mixed], [out])
    torch.cuda.synchronize()
    turned = mixed.cpu().numpy()
    assert np.abs(turned - qpsk * np.exp(1j * offset * np.arange(n))).max() < 1e-4   # the mix really turned it
    y = out.cpu().numpy()[2000:]
    points = np.exp(1j * (np.pi / 2 * np.arange(4) + np.pi / 4))
    dist = np.abs(y[:, None] - points[None, :]).min(axis=1)
    assert dist.max() < 0.1, dist.max()
    assert abs(loop.get_frequency() - offset) < 0.1 * offset


def _pybind():
    import glob
    import importlib.util
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_blocks(gpu):
    mod = _pybind()
    n, amp, ratio = 4099, 1000.5, 0.01234
    src = mod.clSignalSource(idataType=1, openCLPlatformType=1, devSelector=2, platformId=0, devId=0, samp_rate=ref.SIG_SAMP_RATE,
                             waveform=1, freq=ratio * ref.SIG_SAMP_RATE, amplitude=amp)
    inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    y = np.empty(n, np.complex64)
    assert src.work(n, [], [y]) == n
    want, pos = ref.sig_call(0.0, inc, n, amp, "complex", 1)
    _check_sig(y, want, amp)
    assert src.get_angle_pos() == pos and src.get_angle_rate() == inc
    with pytest.raises(ValueError):
        src.work(n, [], [np.empty(n - 1, np.complex64)])
    order, nitems = 4, 4097
    x, _ = ref.costas_input(order, 1, nitems)
    want, want_f, want_state = ref.costas_expected(order, 1, nitems)
    loop = mod.clCostasLoop(openCLPlatformType=1, devSelector=2, platformId=0, devId=0, loop_bw=ref.LOOP_BW, order=order)
    assert (loop.get_alpha(), loop.get_beta()) == ref.costas_gains(ref.LOOP_BW)
    out, f = np.empty(nitems, np.complex64), np.empty(nitems, np.float32)
    assert loop.work(nitems, [x], [out, f]) == nitems
    _check_costas(out, f, want, want_f, x)
    assert abs(loop.get_frequency() - want_state[1][0]) < 1e-6 and abs(loop.get_phase() - want_state[0][0]) < 1e-5   # (float getters)
    with pytest.raises(ValueError):
        mod.clCostasLoop(1, 2, 0, 0, ref.LOOP_BW, 8)   # std::invalid_argument


def test_cli_loops_only(gpu):
    r = subprocess.run([CLI, "--loops-only", "--iterations=5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(rows) == 2 and rows[0].startswith("clSignalSource") and rows[1].startswith("clCostasLoop"), r.stdout
    assert all(l.rstrip().endswith("ok") for l in rows), r.stdout


def test_tuning_variables_are_read_at_create_and_named_in_the_log(gpu, monkeypatch):
    """MI355_SIGSOURCE_LITERAL / MI355_COSTAS_ONE_LANE choose the comparison variant of a handle when it is created, never later
    (tools/loops_probe.py relies on both halves); a debug context names the kernel it chose."""
    def made(make):
        lines = []
        gpu.set_log_callback(lambda level, msg: lines.append(msg))
        try:
            return make(), " | ".join(lines)
        finally:
            gpu.set_log_callback(None)

    n = 4097
    x, _ = ref.costas_input(4, 1, n)
    want, want_f, _ = ref.costas_expected(4, 1, n)
    monkeypatch.delenv("MI355_SIGSOURCE_LITERAL", raising=False)
    monkeypatch.delenv("MI355_COSTAS_ONE_LANE", raising=False)
    src, text = made(lambda: gpu.clSignalSource(1, *GPU_ARGS, 48000.0, 1, 1234.5, 1.0, 1))
    assert "rotation" in text and "literal" not in text
    loop, text = made(lambda: gpu.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, 4, 1))
    assert "k_costas_one" in text
    monkeypatch.setenv("MI355_SIGSOURCE_LITERAL", "1")
    monkeypatch.setenv("MI355_COSTAS_ONE_LANE", "1")
    rot = _gen(src, n, np.complex64)       # created before: still the rotation kernel
    one = _run_loop(loop, x, n)
    src_l, text = made(lambda: gpu.clSignalSource(1, *GPU_ARGS, 48000.0, 1, 1234.5, 1.0, 1))
    assert "literal" in text
    loop_l, text = made(lambda: gpu.clCostasLoop(*GPU_ARGS, ref.LOOP_BW, 4, 1))
    assert "k_costas_lanes" in text
    monkeypatch.delenv("MI355_SIGSOURCE_LITERAL")
    monkeypatch.delenv("MI355_COSTAS_ONE_LANE")
    lit = _gen(src_l, n, np.complex64)     # created with it: the literal kernel, whatever the environment says now
    inc = ref.sig_inc(1234.5, 48000.0)
    want_s, _ = ref.sig_call(0.0, inc, n, 1.0, "complex", 1)
    _check_sig(rot, want_s, 1.0)
    _check_sig(lit, want_s, 1.0)
    lane = _run_loop(loop_l, x, n)
    _check_costas(one[0], one[1], want, want_f, x)
    _check_costas(lane[0], lane[1], want, want_f, x)
    src2 = gpu.clSignalSource(1, *GPU_ARGS, 48000.0, 1, 1234.5, 1.0)   # and with the variables gone: the default again
    assert np.array_equal(_gen(src2, n, np.complex64).view(np.uint32), rot.view(np.uint32))
