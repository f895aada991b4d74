"""clXCorrelate on the device: curves and lags against the float64 oracle (tests/xcorr_td_ref.py), known answers, determinism,
guard bands, the Python mirror's decimation / async schedule, the pybind block and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import xcorr_td_ref as ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
TOL = 5e-5


def _signals(rng, n, k, cplx, nframes=1):
    if cplx:
        return [(rng.standard_normal(nframes * n) + 1j * rng.standard_normal(nframes * n)).astype(np.complex64) for _ in range(k)]
    return [rng.standard_normal(nframes * n).astype(np.float32) for _ in range(k)]


def _block(pkg, k, n, cplx, ms, decim=1, async_=False):
    dt, ds = (pkg.DTYPE_COMPLEX, 8) if cplx else (pkg.DTYPE_FLOAT, 4)
    return pkg.clXCorrelate(*GPU_ARGS, False, k, n, dt, ds, ms, decim, async_)


def _run_dev(blk, ins, nframes, curves=True, stream=None):
    import torch
    nsig, L2 = blk.num_inputs - 1, 2 * blk.max_shift
    d_in = [torch.from_numpy(x).cuda() for x in ins]
    corr = torch.empty(nframes * nsig, dtype=torch.float32, device="cuda")
    lags = torch.empty(nframes * nsig, dtype=torch.int32, device="cuda")
    cv = torch.empty(nframes * nsig * L2, dtype=torch.float32, device="cuda") if curves else None
    if stream is not None:
        with torch.cuda.stream(stream):
            blk.work_device(nframes, d_in, corr, lags, cv)
        stream.synchronize()
    else:
        blk.work_device(nframes, d_in, corr, lags, cv)
        torch.cuda.synchronize()
    out = (corr.cpu().numpy().reshape(nframes, nsig), lags.cpu().numpy().reshape(nframes, nsig))
    return out + ((cv.cpu().numpy().reshape(nframes, nsig, L2),) if curves else (None,))


def _check_lag(ref_curve, got_corr, got_lag, m):
    best, lag = ref.find_max(ref_curve, m)
    order = np.sort(ref_curve[np.isfinite(ref_curve)])
    if len(order) < 2 or order[-1] - order[-2] > 1e-4:
        assert got_lag == lag, (got_lag, lag)
    else:
        assert ref_curve[got_lag + m] >= best - 1e-4, (got_lag, lag)
    assert abs(got_corr - best) <= TOL


CASES = [  # (complex, N, max_search_index, num_inputs, frames)
    (True, 2, 2, 2, 3), (False, 2, 2, 3, 2), (True, 6, 6, 2, 2), (False, 300, 300, 3, 2), (True, 300, 6, 2, 1),
    (False, 1000, 0, 2, 2), (True, 4096, 2, 3, 2), (False, 8192, 6000, 2, 1), (True, 8192, 512, 32, 1), (False, 2048, 300, 32, 1),
    (True, 65536, 300, 2, 1), (False, 65536, 6, 3, 1), (True, 40000, 0, 2, 1),
]


@pytest.mark.parametrize("cplx,n,ms,k,nf", CASES)
def test_curves_and_lags_against_float64(gpu, cplx, n, ms, k, nf):
    rng = np.random.default_rng(n + 7 * ms + k)
    blk = _block(gpu, k, n, cplx, ms)
    m = blk.max_shift
    assert m == ref.plan(n, ms)
    ins = _signals(rng, n, k, cplx, nf)
    corr, lags, cv = _run_dev(blk, ins, nf)
    for f in range(nf):
        for s in range(1, k):
            x, y = ins[0][f * n:(f + 1) * n], ins[s][f * n:(f + 1) * n]
            rc = ref.curve_literal(x, y, m) if n * m <= 4096 else ref.curve(x, y, m)
            got = cv[f, s - 1]
            assert np.array_equal(got == -2.0, rc == -2.0), (f, s)
            err = np.abs(got.astype(np.float64) - rc).max()
            assert err <= TOL, (f, s, err)
            _check_lag(rc, corr[f, s - 1], lags[f, s - 1], m)


def test_large_shape_one_frame(gpu):
    """2^20 items, max search 4096, 4 complex inputs."""
    n, k = 1 << 20, 4
    rng = np.random.default_rng(11)
    blk = _block(gpu, k, n, True, 4096)
    ins = _signals(rng, n, k, True)
    ins[2] = np.roll(ins[0], 1234) + 0.5 * ins[2]  # a delayed copy under noise: lag -1234
    corr, lags, cv = _run_dev(blk, ins, 1)
    for s in range(1, k):
        rc = ref.curve(ins[0], ins[s], blk.max_shift)
        assert np.abs(cv[0, s - 1] - rc).max() <= TOL, s
        _check_lag(rc, corr[0, s - 1], lags[0, s - 1], blk.max_shift)
    assert lags[0, 1] == -1234


@pytest.mark.parametrize("cplx", [True, False])
def test_delayed_copies_and_zero_inputs(gpu, cplx):
    n = 8192
    rng = np.random.default_rng(3)
    base = _signals(rng, n + 600, 1, cplx)[0]
    x = base[300:300 + n]
    ins = [x] + [base[300 - d:300 - d + n] for d in (-300, 0, 1, 257)]   # y[j] = x[j - d]: delayed by d
    blk = _block(gpu, len(ins), n, cplx, 512)
    corr, lags = np.empty(4, np.float32), np.empty(4, np.int32)
    assert blk._L.mi355_xcorr_td_work(blk._h, (gpu.blocks.C.c_void_p * 5)(*[x.ctypes.data for x in ins]),
                                      corr.ctypes.data, lags.ctypes.data) == 0
    assert list(lags) == [300, 0, -1, -257] and np.abs(corr - 1.0).max() < 1e-5, (lags, corr)
    zero = np.zeros(n, ins[0].dtype)
    assert blk.work(n, [zero] * 5) == n
    pdu = blk.pop_pdu()
    assert np.all(pdu["corrvect"] == -2.0) and np.all(pdu["corrective_lags"] == -blk.max_shift)


def test_batches_streams_and_repeats_are_bit_identical(gpu):
    import torch
    n, k, nf = 3000, 3, 5
    rng = np.random.default_rng(5)
    blk = _block(gpu, k, n, True, 0)
    ins = _signals(rng, n, k, True, nf)
    batch = _run_dev(blk, ins, nf)
    again = _run_dev(blk, ins, nf, stream=torch.cuda.Stream())
    for a, b in zip(batch, again):
        assert np.array_equal(a, b)
    for f in range(nf):
        one = _run_dev(blk, [x[f * n:(f + 1) * n].copy() for x in ins], 1)
        for a, b in zip(batch, one):
            assert np.array_equal(a[f], b[0])


def test_guard_bands(gpu):
    """NaN pads around every input frame region and sentinel words around every output: nothing outside is read or written."""
    import torch
    n, k, nf, pad = 1000, 3, 2, 4096
    rng = np.random.default_rng(9)
    blk = _block(gpu, k, n, False, 0)
    m, nsig = blk.max_shift, k - 1
    ins = _signals(rng, n, k, False, nf)
    clean = _run_dev(blk, ins, nf)
    bufs, views = [], []
    for x in ins:
        b = torch.full((pad + nf * n + pad,), float("nan"), dtype=torch.float32, device="cuda")
        b[pad:pad + nf * n] = torch.from_numpy(x).cuda()
        bufs.append(b)
        views.append(b[pad:pad + nf * n])
    sent = 64

    def guarded(count, dtype, fill):
        g = torch.full((sent + count + sent,), fill, dtype=dtype, device="cuda")
        return g, g[sent:sent + count]

    cg, cv_ = guarded(nf * nsig, torch.float32, 12345.0)
    lg, lv = guarded(nf * nsig, torch.int32, 0x5A5A5A5A)
    vg, vv = guarded(nf * nsig * 2 * m, torch.float32, -777.0)
    blk.work_device(nf, views, cv_, lv, vv)
    torch.cuda.synchronize()
    for g, fill in ((cg, 12345.0), (lg, 0x5A5A5A5A), (vg, -777.0)):
        h = g.cpu().numpy()
        assert np.all(h[:sent] == fill) and np.all(h[-sent:] == fill)
    assert np.array_equal(cv_.cpu().numpy().reshape(nf, nsig), clean[0])
    assert np.array_equal(lv.cpu().numpy().reshape(nf, nsig), clean[1])
    assert np.array_equal(vv.cpu().numpy().reshape(nf, nsig, 2 * m), clean[2])


def _frames_with_delays(rng, n, delays, cplx=True):
    """One frame per delay: input 1 is input 0 delayed by delays[f] (expected lag -delays[f])."""
    frames = []
    for d in delays:
        base = _signals(rng, n + 64, 1, cplx)[0]
        frames.append([base[32:32 + n], base[32 - d:32 - d + n]])
    return frames


def test_mirror_decimation(gpu):
    n = 2048
    rng = np.random.default_rng(1)
    delays = [1, 2, 3, 4, 5, 6, 7]
    blk = _block(gpu, 2, n, True, 64, decim=3)
    for fr in _frames_with_delays(rng, n, delays):
        assert blk.work(n, fr) == n
    got = []
    while True:
        p = blk.pop_pdu()
        if p is None:
            break
        got.append(int(p["corrective_lags"][0]))
        assert p["corrvect"].dtype == np.float32 and p["corrective_lags"].dtype == np.int32
    assert got == [-3, -6]  # frames 2 and 5
    assert blk.work(n - 1, _frames_with_delays(rng, n, [0])[0]) == 0


def test_mirror_async_schedule(gpu):
    n = 2048
    rng = np.random.default_rng(2)
    delays = [3, 5, 7, 9]
    blk = _block(gpu, 2, n, True, 64, async_=True)
    for k, fr in enumerate(_frames_with_delays(rng, n, delays)):
        assert blk.work(n, fr) == n
        p = blk.pop_pdu()
        if k == 0:
            assert p is None
        else:
            assert int(p["corrective_lags"][0]) == -delays[k - 1] and abs(float(p["corrvect"][0]) - 1.0) < 1e-5
        assert blk.pop_pdu() is None
        blk.wait()
    blk.stop()  # the last frame's result is dropped
    assert blk.pop_pdu() is None


def test_pybind_block_as_a_flowgraph_builds_it(gpu):
    import importlib.util
    import glob
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    n = 8192
    b = mod.clXCorrelate(1, 2, 0, 0, False, 2, n, 1, 8, 512, 4, True)
    assert b.max_shift() == 512
    rng = np.random.default_rng(4)
    fr = _frames_with_delays(rng, n, [11])[0]
    for _ in range(9):
        assert b.work(n, fr) == n
        b.wait()
    pdus = b.pop_pdus()
    assert len(pdus) >= 1 and all(int(l[0]) == -11 for _, l in pdus), pdus


def test_cli_xcorrelate_only(gpu):
    r = subprocess.run([CLI, "--xcorrelate-only", "--iterations=5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "clXCorrelate" in r.stdout and r.stdout.rstrip().endswith("ok"), r.stdout
