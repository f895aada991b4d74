"""GPU: clRationalResampler / clInterpFIRFilter against tests/resampler_ref.py.  One tolerance, ref.bound(): derived from the float32
dot product an output is, not fitted.  Every output of every case is compared; one handle per (rate, taps), the call sizes and the
phases loop inside a test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import guarded
import resampler_ref as ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
NMAX = max(ref.NOUT)
GRID = [(c, False) for c in ref.grid()] + [((L, M, K), True) for L, M in ref.COMPLEX_RATES for K in ref.ks(L)]


def _gid(v):
    return ref.case_id(v[0]) + ("-ccc" if v[1] else "")


def _run(blk, x, n, phase):
    """work_device on a NaN-filled output from `phase`; x: a numpy array or a tensor holding the history-prefixed input"""
    import torch
    d_in = torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x
    d_out = torch.full((n,), float("nan"), dtype=torch.complex64, device="cuda")
    blk.set_phase(phase)
    got_n, used = blk.work_device(n, [d_in], [d_out])
    assert got_n == n
    return d_out.cpu().numpy(), used


@pytest.mark.parametrize("case", GRID, ids=_gid)
def test_grid(gpu, case):
    import torch
    (L, M, K), cplx = case
    h = ref.make_taps(K, cplx)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h)
    assert blk.history() == ref.taps_per_arm(K, L) and blk.interpolation() == L and blk.decimation() == M
    assert np.array_equal(blk.taps(), h)
    for c in ref.phases(L):
        x = ref.make_input(L, M, K, c, NMAX)
        want = ref.resample(h, L, M, x, NMAX, c)[0]
        bnd = ref.bound(h, L, x, c, M, NMAX)
        d_x = torch.from_numpy(x).cuda()
        for n in ref.NOUT:
            _, used, need, c2 = ref.plan(L, M, K, c, n)
            blk.set_phase(c)
            assert blk.plan(n) == (used, need, c2)
            got, got_used = _run(blk, d_x[:need].clone(), n, c)  # exactly `needed` items
            assert got_used == used and blk.phase() == c2, (c, n)
            assert ref.within(got, want[:n], bnd[:n]), (c, n, ref.worst(got, want[:n], bnd[:n]))
            blk.set_phase(c)
            assert blk.noutput_for(need) >= n > blk.noutput_for(need - 1)
    blk.stop()


@pytest.mark.parametrize("case", [(8, 1, 89), (3, 2, 391), (5, 7, 3), (160, 147, 3840)], ids=ref.case_id)
def test_any_split_gives_the_same_bits(gpu, case):
    import torch
    L, M, K = case
    h = ref.rrc(8.0, 8, 0.35, 89) if case == (8, 1, 89) else ref.make_taps(K)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h)
    x = ref.make_input(L, M, K, 0, NMAX)
    d_x = torch.from_numpy(x).cuda()
    whole, used_whole = _run(blk, d_x, NMAX, 0)
    assert ref.within(whole, ref.resample(h, L, M, x, NMAX, 0)[0], ref.bound(h, L, x, 0, M, NMAX))
    rng = np.random.default_rng(5)
    blk.set_phase(0)
    d_out = torch.full((NMAX,), float("nan"), dtype=torch.complex64, device="cuda")
    done, pos, c = 0, 0, 0
    while done < NMAX:
        n = min(int(rng.choice([0, 1, 2, 17, 64, 1000, 4097])), NMAX - done)
        _, used, need, c2 = ref.plan(L, M, K, c, n)
        assert blk.work_device(n, [d_x[pos:pos + max(need, 1)]], [d_out[done:done + max(n, 1)]]) == (n, used)
        assert blk.phase() == c2
        done, pos, c = done + n, pos + used, c2     # in += consumed
    assert pos == used_whole
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    blk.stop()


@pytest.mark.parametrize("case", [(8, 1, 89), (3, 2, 13), (2, 3, 13), (160, 147, 3840)], ids=ref.case_id)
def test_guard_bands_and_alignment(gpu, case):
    import torch
    L, M, K = case
    h = ref.make_taps(K)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h)
    pad = guarded.pad_items(8)
    for n in (257, NMAX):
        x = ref.make_input(L, M, K, L // 2, n)
        want = ref.resample(h, L, M, x, n, L // 2)[0]
        bnd = ref.bound(h, L, x, L // 2, M, n)
        res = []
        for off in (0, 1):  # 16-byte aligned, and 8-byte aligned only
            wi, vi = guarded.guarded_input(x, pad, off, device="cuda")
            wo, vo = guarded.guarded_output(n, np.complex64, pad, off, device="cuda")
            blk.set_phase(L // 2)
            blk.work_device(n, [vi], [vo])
            torch.cuda.synchronize()
            guarded.check_guards(wi, vi, "input")
            guarded.check_guards(wo, vo, "output")
            res.append(guarded.to_numpy(vo))
            assert ref.within(res[-1], want, bnd), (n, off)
        assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32)), n
    blk.stop()


@pytest.mark.parametrize("case", [(8, 1, 89), (3, 2, 13), (1, 3, 11)], ids=ref.case_id)
def test_window_locality(gpu, case):
    """One NaN at an interior sample s: exactly the outputs whose window [b, b + nt) holds s are NaN (also under a zero tap of a
    padded arm), all others keep their bits."""
    L, M, K = case
    n, c = 257, 0
    h = ref.make_taps(K)
    nt = ref.taps_per_arm(K, L)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h)
    x = ref.make_input(L, M, K, c, n)
    clean, _ = _run(blk, x, n, c)
    s = x.size // 2
    x2 = x.copy()
    x2[s] = complex(np.nan, np.nan)
    dirty, _ = _run(blk, x2, n, c)
    b = (c + np.arange(n) * M) // L
    hit = (b <= s) & (s < b + nt)
    assert 0 < hit.sum() < n
    assert np.array_equal(np.isnan(dirty.real) | np.isnan(dirty.imag), hit)
    assert np.all(np.isnan(dirty[hit].real) & np.isnan(dirty[hit].imag))
    assert np.array_equal(dirty[~hit].view(np.uint32), clean[~hit].view(np.uint32))
    blk.stop()


def _zero_stuffed(x_hist, nt, L, K):
    """the history-prefixed input of clFilter(decimation M, the K taps) that yields the same outputs: the zero-stuffed stream with
    K - 1 items of history in front of L x[0]"""
    z = np.zeros(x_hist.size * L, np.complex64)
    z[::L] = x_hist
    start = (nt - 1) * L - (K - 1)  # z[(nt-1) L] is x[0]
    return np.concatenate([np.zeros(-start, np.complex64), z]) if start < 0 else z[start:]


@pytest.mark.parametrize("case", [(8, 1, 89), (3, 2, 97)], ids=ref.case_id)
def test_against_the_zero_stuffed_clfilter(gpu, case):
    L, M, K = case
    n = NMAX
    h = ref.make_taps(K)
    x = ref.make_input(L, M, K, 0, n)
    want = ref.resample(h, L, M, x, n, 0)[0]
    bnd = ref.bound(h, L, x, 0, M, n)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h)
    got, _ = _run(blk, x, n, 0)
    assert ref.within(got, want, bnd)
    z = _zero_stuffed(x, ref.taps_per_arm(K, L), L, K)
    z = np.concatenate([z, np.zeros(max(0, n * M + K - 1 - z.size), np.complex64)])
    fil = gpu.clFilter(*GPU_ARGS, M, h, 1, 0, True)
    y = np.empty(n, np.complex64)
    fil.work(n, [z], [y])
    assert ref.within(y, want, bnd), ref.worst(y, want, bnd)
    blk.stop()


@pytest.mark.parametrize("case", [(1, 1, 65), (1, 3, 11)], ids=ref.case_id)
def test_degenerate_rates_agree_with_clfilter(gpu, case):
    L, M, K = case
    n = 4099
    h = ref.make_taps(K)
    x = ref.make_input(L, M, K, 0, n)
    got, _ = _run(gpu.clRationalResampler(*GPU_ARGS, L, M, h), x, n, 0)
    y = np.empty(n, np.complex64)
    xf = np.concatenate([x, np.zeros(M - 1, np.complex64)])  # clFilter asks for n M + K - 1 items; no output reads the last M - 1
    gpu.clFilter(*GPU_ARGS, M, h, 1, 0, True).work(n, [xf], [y])
    bnd = ref.bound(h, L, x, 0, M, n)
    assert ref.within(got, y.astype(np.complex128), 2 * bnd)
    assert ref.within(got, ref.resample(h, L, M, x, n, 0)[0], bnd)


@pytest.mark.parametrize("case,n", [((8, 1, 89), 4099), ((3, 2, 97), 1 << 20 | 77), ((2, 3, 13), 70001)], ids=str)
def test_host_pointer_work(gpu, case, n):
    """work() on numpy buffers; the second shape writes more than 8 MiB of output and is staged in several pieces"""
    L, M, K = case
    c = L // 2
    h = ref.make_taps(K)
    x = ref.make_input(L, M, K, c, n)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h) if M != 1 else gpu.clInterpFIRFilter(*GPU_ARGS, L, h)
    blk.set_phase(c)
    y = np.full(n, np.nan, np.complex64)
    _, used, need, c2 = ref.plan(L, M, K, c, n)
    assert blk.work(n, [x], [y]) == (n, used) and blk.phase() == c2
    assert ref.within(y, ref.resample(h, L, M, x, n, c)[0], ref.bound(h, L, x, c, M, n))
    with pytest.raises(ValueError):
        blk.work(n, [x[:need - 1]], [y])
    blk.stop()


def test_set_taps_between_enqueued_calls(gpu):
    """two work_device calls on one stream with set_taps (24 -> 36 taps: the history changes) between them and no synchronisation:
    the old taps entirely, then the new, from the phase the first call left"""
    import torch
    L, M, n = 3, 2, 2000
    h1, h2 = ref.make_taps(24), ref.make_taps(36, seed=1)
    c2 = ref.plan(L, M, 24, 0, n)[3]
    x1, x2 = ref.make_input(L, M, 24, 0, n), ref.make_input(L, M, 36, c2, n, seed=1)
    blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h1)
    d_x1, d_x2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    o1 = torch.full((n,), float("nan"), dtype=torch.complex64, device="cuda")
    o2 = torch.full_like(o1, float("nan"))
    torch.cuda.synchronize()
    assert blk.work_device(n, [d_x1], [o1])[0] == n and blk.phase() == c2
    blk.set_taps(h2)
    assert blk.work_device(n, [d_x2], [o2])[0] == n
    torch.cuda.synchronize()
    assert ref.within(o1.cpu().numpy(), ref.resample(h1, L, M, x1, n, 0)[0], ref.bound(h1, L, x1, 0, M, n))
    assert ref.within(o2.cpu().numpy(), ref.resample(h2, L, M, x2, n, c2)[0], ref.bound(h2, L, x2, c2, M, n))
    blk.stop()


def test_handle_behaviour(gpu):
    import torch
    L, M = 3, 2
    h1, h2 = ref.make_taps(13), ref.make_taps(31, seed=1)
    got = []
    gpu.set_log_callback(lambda level, msg: got.append((level, msg)))
    try:
        blk = gpu.clRationalResampler(*GPU_ARGS, L, M, h1, 1)
        big = gpu.clRationalResampler(*GPU_ARGS, 65536, 1, ref.make_taps(5), 1)  # 65536 arms: beyond the LDS form
    finally:
        gpu.set_log_callback(None)
    info = [m for lvl, m in got if lvl == 1 and m.startswith("clRationalResampler:")]
    assert len(info) == 2 and "k_rs_lds" in info[0] and "13 real taps (5 per arm)" in info[0] and "k_rs_plain" in info[1], got
    # the fallback kernel computes the same thing
    xb = ref.make_input(65536, 1, 5, 65535, 70000)
    yb, _ = _run(big, xb, 70000, 65535)
    assert ref.within(yb, ref.resample(ref.make_taps(5), 65536, 1, xb, 70000, 65535)[0], ref.bound(ref.make_taps(5), 65536, xb, 65535, 1, 70000))
    # set_taps mid-stream: the phase is kept, the history changes
    x = ref.make_input(L, M, 31, 0, 1000)
    blk.work_device(100, [torch.from_numpy(x).cuda()], [torch.empty(100, dtype=torch.complex64, device="cuda")])
    c = blk.phase()
    assert c == (100 * M) % L and blk.history() == 5
    blk.set_taps(h2)
    assert blk.phase() == c and blk.history() == 11 and np.array_equal(blk.taps(), h2)
    y, _ = _run(blk, x, 500, c)
    assert ref.within(y, ref.resample(h2, L, M, x, 500, c)[0], ref.bound(h2, L, x, c, M, 500))
    with pytest.raises(TypeError):
        blk.set_taps(h2.astype(np.complex64) * 1j)
    with pytest.raises(gpu.Mi355Error):
        blk.set_phase(L)
    # in == out (any overlap) is refused; n == 0 is a no-op; a short input is refused before the launch
    buf = torch.from_numpy(x).cuda()
    c = blk.phase()
    need = blk.plan(100)[1]
    for src, out in ((buf, buf), (buf, buf[7:]), (buf, buf[need - 1:]), (buf[99:], buf)):
        with pytest.raises(gpu.Mi355Error) as e:
            blk.work_device(100, [src], [out])
        assert e.value.code == -1 and blk.phase() == c
    assert blk.work_device(100, [buf], [buf[need:]])[0] == 100  # the same allocation, no overlap
    blk.set_phase(c)
    assert blk.work_device(0, [buf[:0]], [buf[:0]]) == (0, 0) and blk.phase() == c
    assert blk.work(0, [x[:0]], [np.empty(0, np.complex64)]) == (0, 0)
    with pytest.raises(ValueError):
        blk.work_device(100, [buf[:need - 1]], [torch.empty(100, dtype=torch.complex64, device="cuda")])
    with pytest.raises(ValueError):
        blk.work_device(100, [buf], [torch.empty(99, dtype=torch.complex64, device="cuda")])
    torch.cuda.synchronize()
    with pytest.raises(gpu.Mi355Error) as e:
        gpu.clRationalResampler(*GPU_ARGS, 65536, 1, np.ones(16 * 65536 + 1, np.float32))
    assert e.value.code == -3
    blk.stop()
    big.stop()


def _pybind():
    import glob
    import importlib.util
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("cplx", [False, True], ids=["ccf", "ccc"])
def test_pybind_block_over_uneven_pieces(gpu, cplx):
    """general_work() as the scheduler calls it: whatever input there is (history included) is offered, the block produces what
    that allows and consumes accordingly; the pieces together are one resample() of the whole stream."""
    mod = _pybind()
    L, M, K = 7, 5, 31
    h = ref.make_taps(K, cplx)
    if cplx:
        blk = mod.clRationalResampler.make_ccc(*GPU_ARGS, L, M, h.tolist())
    else:
        blk = mod.clRationalResampler(*GPU_ARGS, L, M, h.tolist())
    nt = ref.taps_per_arm(K, L)
    assert blk.history() == nt and blk.interpolation() == L and blk.decimation() == M
    assert np.array_equal(np.asarray(blk.taps(), np.complex64), h.astype(np.complex64))
    assert blk.forecast(100) == ref.plan(L, M, K, 0, 100)[2]
    total = 9000
    x = ref.crandn(np.random.default_rng(3), nt - 1 + total)
    y = np.full(total * L // M + 8, np.nan, np.complex64)
    rng = np.random.default_rng(4)
    pos, made, c = 0, 0, 0
    for _ in range(2000):
        if ref.noutput_for(L, M, K, c, x.size - pos) == 0:
            break
        avail = min(int(rng.choice([nt - 1, nt, nt + 1, 64, 1000, 4097])), x.size - pos)  # items from the read pointer on
        room = min(int(rng.choice([1, 3, 500, 10000])), y.size - made)
        want_n = min(ref.noutput_for(L, M, K, c, avail), room)
        produced, consumed = blk.general_work(room, [x[pos:pos + avail]], [y[made:made + room]])
        assert (produced, consumed) == (want_n, ref.plan(L, M, K, c, want_n)[1])
        c = ref.plan(L, M, K, c, want_n)[3]
        pos, made = pos + consumed, made + produced
    assert ref.noutput_for(L, M, K, c, x.size - pos) == 0
    assert made > 10000
    want = ref.resample(h, L, M, x, made, 0)[0]
    assert ref.within(y[:made], want, ref.bound(h, L, x, 0, M, made))


def test_cli_resampler_only():
    r = subprocess.run([CLI, "--resampler-only", "--iterations=5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(rows) == 2 and all(l.startswith("clRationalResampler") and l.rstrip().endswith("ok") for l in rows), r.stdout
