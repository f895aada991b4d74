"""GPU: clPolyphaseSynthesizer against tests/synth_ref.py (float64, rounded to float).  One tolerance, conftest.relerr <= ref.TOL =
1e-5 (DESIGN.md "Tolerances", the channelizer's value for the same transform + FIR structure).  Every output of every case is
compared; one handle per shape, the call sizes loop inside a test; the output is NaN before every call.

Routes and their limits, as csrc/synth.hip and csrc/fft_mr.hip state them:
  fused pow2         M = 8 .. 4096 a power of two, tile F = 4096 / M frames, ring of at most 5 regions: T <= 4 F + 1 = 16384 / M + 1
  fused mixed-radix  M = 2^a 3^b 5^c 7^d 11^e 13^f with at least two factors that is no power of two (the lengths MrPlan takes: 6, 10, 12, 100
                     ... but not 3, 5 or 7), while a ring of 1 + ceil((T - 1) / F) padded tiles fits
                     160 KiB; at M = 4095 one frame is 4095 + 127 + 1 slots = 33784 bytes, four fit: T <= 4
  generic            everything else: M = 1 .. 5 and 7, larger prime factors, T past the ring, MI355_SYNTH_GENERIC=1
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT, relerr
import guarded
import synth_ref as ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
MS = (1, 2, 3, 4, 7, 8, 10, 12, 16, 32, 64, 100, 128, 256, 512, 1024, 4096, 4095)
KINDS = ("ident", "perm", "half", "one")
GENERIC_F = 16  # the generic route has no tile; the call sizes of its cases are built around this


def expected_route(M, T):
    if M >= 8 and M & (M - 1) == 0:
        return "fused pow2" if T <= 16384 // M + 1 else "generic"
    if M in (10, 12, 100):
        return "fused mixed-radix"  # (their rings hold hundreds of frames)
    if M == 4095:
        return "fused mixed-radix" if T <= 4 else "generic"
    return "generic"


def tile_of(route):
    m = re.search(r"tile=(\d+)", route)
    return int(m.group(1)) if m else GENERIC_F


def _run(blk, d_x, nframes, M):
    """work_device on a NaN-filled output"""
    import torch
    d_out = torch.full((max(nframes * M, 1),), float("nan"), dtype=torch.complex64, device="cuda")
    assert blk.work_device(nframes, [d_x], [d_out]) == nframes * M
    return d_out.cpu().numpy()[:nframes * M]


def _ts(M):
    ts = [1, 2, 3, 8]
    if M in (1024, 4096):
        ts.append(16384 // M + 2)  # one past what the pow2 ring holds: 18, 6
    if M == 4095:
        ts.append(5)               # one past what the mixed-radix ring holds
    return ts


@pytest.mark.parametrize("M", MS)
def test_grid(gpu, M):
    """T in {1, 2, 3, 8} and one past each fused ring; K = T M and K = T M - (M // 2 + 1) alternate and the four maps rotate over
    the T of a channel count, shifted per M, so every M sees both tap forms and every map; nframes in {1, 2, F-1, F, F+1, 3F+5}
    on the prefix of one stream (the outputs of a shorter call are a prefix of the longer one's)."""
    import torch
    for ti, T in enumerate(_ts(M)):
        K = T * M if (ti + M) % 2 == 0 else max(T * M - (M // 2 + 1), (T - 1) * M + 1)
        kind = KINDS[(ti + M) % 4]
        m = ref.make_map(M, kind, seed=T)
        nmap = ref.nmap_of(M, m)
        g = ref.make_taps(K, seed=M + T)
        blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g, M, m)
        route = blk.route()
        assert route.startswith(expected_route(M, T)), (M, T, route)
        assert blk.taps_per_arm() == T == ref.taps_per_arm(K, M) and blk.history() == (T - 1) * nmap
        assert np.array_equal(blk.taps(), g)
        F = tile_of(route)
        nmax = 3 * F + 5
        x = ref.make_input(K, M, nmap, nmax, seed=M)
        want = ref.synth(g, M, m, x, nmax).astype(np.complex64)
        d_x = torch.from_numpy(x).cuda()
        for n in sorted({1, 2, max(F - 1, 1), F, F + 1, nmax}):
            nin, nout = ref.plan(K, M, nmap, n)[1:]
            assert blk.plan(n) == (nin, nout)
            got = _run(blk, d_x[:nin].clone(), n, M)  # exactly the items the call may read
            assert np.all(np.isfinite(got.view(np.float32))), (M, T, kind, n)
            e = relerr(got, want[:nout])
            assert e <= ref.TOL, (M, T, K, kind, n, route, e)
        blk.stop()


def test_every_route_is_reached(gpu):
    for M, T, name in ((64, 8, "fused pow2 M=64 T=8 tile=64"), (4096, 5, "fused pow2 M=4096 T=5 tile=1"), (8, 2049, "fused pow2 M=8 T=2049 tile=512"),
                       (12, 4, "fused mixed-radix M=12 T=4 tile=64"), (1, 5, "generic"), (17, 2, "generic"), (4096, 6, "generic"), (8, 2050, "generic"),
                       (4095, 5, "generic")):
        blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, ref.make_taps(T * M), M)
        assert blk.route() == name, (M, T, blk.route())
        blk.stop()
    blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, ref.make_taps(4 * 4095), 4095)
    assert blk.route().startswith("fused mixed-radix M=4095 T=4 tile="), blk.route()
    blk.stop()


# one shape per route for the structural tests: (M, T, map kind)
ROUTE_SHAPES = [(64, 8, "ident"), (64, 8, "half"), (12, 4, "perm"), (100, 3, "ident"), (3, 3, "perm"), (4096, 6, "ident")]


@pytest.mark.parametrize("M,T", [(64, 8), (12, 4)], ids=["pow2", "mixed-radix"])
def test_persistent_loop(gpu, M, T):
    """More tiles than the launch has workgroups (at most 4 per CU for the pow2 kernel, 8 for the mixed-radix one at 256 threads), so
    every workgroup walks a run of several tiles and hands the ring over between them."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = ref.make_taps(T * M)
    blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g, M)
    F = tile_of(blk.route())
    assert blk.route().startswith("fused")
    n = ((4 if M == 64 else 8) * cus + 7) * F + 3
    x = ref.make_input(T * M, M, M, n)
    got = _run(blk, torch.from_numpy(x).cuda(), n, M)
    e = relerr(got, ref.synth(g, M, None, x, n).astype(np.complex64))
    assert e <= ref.TOL, e
    blk.stop()


@pytest.mark.parametrize("case", ROUTE_SHAPES, ids=ref.case_id)
def test_any_split_gives_the_same_bits(gpu, case):
    import torch
    M, T, kind = case
    K = T * M - 1
    m = ref.make_map(M, kind)
    nmap = ref.nmap_of(M, m)
    g = ref.make_taps(K)
    blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g, M, m)
    F = tile_of(blk.route())
    total = 6 * F + 41
    x = ref.make_input(K, M, nmap, total)
    d_x = torch.from_numpy(x).cuda()
    whole = _run(blk, d_x, total, M)
    assert relerr(whole, ref.synth(g, M, m, x, total).astype(np.complex64)) <= ref.TOL
    rng = np.random.default_rng(5)
    d_out = torch.full((total * M,), float("nan"), dtype=torch.complex64, device="cuda")
    done = 0
    while done < total:
        n = min(int(rng.choice([0, 1, 2, 17, F, F + 1])), total - done)
        nin = ref.plan(K, M, nmap, n)[1]
        src = d_x[done * nmap:done * nmap + max(nin, 1)]  # in += nframes nmap
        assert blk.work_device(n, [src], [d_out[done * M:done * M + max(n * M, 1)]]) == n * M
        done += n
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), whole.view(np.uint32))
    blk.stop()


@pytest.mark.parametrize("case", ROUTE_SHAPES, ids=ref.case_id)
def test_guard_bands_and_alignment(gpu, case):
    """a call reads exactly (T - 1 + nframes) nmap items and writes exactly nframes M, at 16-byte and at 8-byte-only alignment, and
    the two give the same bits"""
    import torch
    M, T, kind = case
    K = T * M - (M // 2 + 1)
    m = ref.make_map(M, kind)
    nmap = ref.nmap_of(M, m)
    g = ref.make_taps(K)
    blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g, M, m)
    F = tile_of(blk.route())
    pad = guarded.pad_items(8)
    for n in (1, 2 * F + 3):
        x = ref.make_input(K, M, nmap, n)
        want = ref.synth(g, M, m, x, n).astype(np.complex64)
        res = []
        for off in (0, 1):
            wi, vi = guarded.guarded_input(x, pad, off, device="cuda")
            wo, vo = guarded.guarded_output(n * M, np.complex64, pad, off, device="cuda")
            blk.work_device(n, [vi], [vo])
            torch.cuda.synchronize()
            guarded.check_guards(wi, vi, "input")
            guarded.check_guards(wo, vo, "output")
            res.append(guarded.to_numpy(vo))
            assert relerr(res[-1], want) <= ref.TOL, (n, off)
        assert np.array_equal(res[0].view(np.uint32), res[1].view(np.uint32)), n
    blk.stop()


@pytest.mark.parametrize("case", ROUTE_SHAPES, ids=ref.case_id)
def test_locality(gpu, case):
    """One NaN in one slot of input frame fi (counted in the history-prefixed stream): V of that frame is NaN at every phase, so
    exactly the outputs of frames fi - T + 1 .. fi are non-finite and every other output keeps its bits.  With K = T M no tap is zero,
    so all M phases of those frames are hit.  With a padded last arm the zero taps of lag T - 1 still meet the NaN -- 0 x NaN is NaN in
    the chain the contract prescribes -- so there the hit set is checked from both sides: every output with a non-zero tap at its lag
    is non-finite, and nothing outside the T frames is."""
    import torch
    M, T, kind = case
    m = ref.make_map(M, kind)
    nmap = ref.nmap_of(M, m)
    for K in (T * M, T * M - (M // 2 + 1)):
        g = ref.make_taps(K)
        blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g, M, m)
        F = tile_of(blk.route())
        n = 2 * F + T + 3
        x = ref.make_input(K, M, nmap, n)
        clean = _run(blk, torch.from_numpy(x).cuda(), n, M)
        fi = T - 1 + F  # the newest frame of output frame F: the first of the second tile, its window reaches back into the first
        x2 = x.copy()
        x2[fi * nmap + nmap // 2] = complex(np.nan, np.nan)
        dirty = _run(blk, torch.from_numpy(x2).cuda(), n, M)
        bad = ~(np.isfinite(dirty.real) & np.isfinite(dirty.imag)).reshape(n, M)
        frames = np.zeros((n, M), bool)
        frames[max(fi - T + 1, 0):fi + 1] = True  # output l reads input frames l .. l + T - 1
        gp = np.zeros(T * M, np.float32)
        gp[:K] = g
        nonzero = np.zeros((n, M), bool)
        for l in range(max(fi - T + 1, 0), min(fi, n - 1) + 1):
            nonzero[l] = gp.reshape(T, M)[l + T - 1 - fi] != 0
        assert 0 < frames.sum() < n * M
        assert np.all(bad[nonzero]) and not np.any(bad[~frames]), (K, int(bad.sum()), int(frames.sum()))
        if K == T * M:
            assert np.array_equal(bad, frames) and np.array_equal(nonzero, frames)
        keep = ~frames.reshape(-1)
        assert np.array_equal(dirty[keep].view(np.uint32), clean[keep].view(np.uint32))
        blk.stop()


@pytest.mark.parametrize("M", [4, 64, 12])
def test_round_trip_with_the_channelizer_on_the_device(gpu, M):
    """clPolyphaseChannelizer(h = ones(M)) -> clPolyphaseSynthesizer(g = [0, 1/M ...]): the channelizer's output tensor goes
    straight into work_device behind one zero frame of history; y[0] = 0, y[n] = x_hist[n - 1]."""
    import torch
    nsteps = 256
    rng = np.random.default_rng(M)
    x_hist = (rng.standard_normal(nsteps * M) + 1j * rng.standard_normal(nsteps * M)).astype(np.complex64)
    ana = gpu.clPolyphaseChannelizer(*GPU_ARGS, np.ones(M, np.float32), nsteps * M, M, M, np.arange(M, dtype=np.int32))
    syn = gpu.clPolyphaseSynthesizer(*GPU_ARGS, np.concatenate([[0.0], np.full(M, 1.0 / M)]).astype(np.float32), M)
    assert ana.ninput() == x_hist.size and ana.noutput() == nsteps * M and syn.history() == M
    d_u = torch.zeros((1 + nsteps) * M, dtype=torch.complex64, device="cuda")
    ana.work_device([torch.from_numpy(x_hist).cuda()], [d_u[M:]])
    y = _run(syn, d_u, nsteps, M)
    assert abs(y[0]) <= ref.TOL * float(np.abs(x_hist).max())
    assert relerr(y[1:], x_hist[:-1]) <= ref.TOL
    ana.stop()
    syn.stop()


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import __graft_entry__ as entry
import synth_ref as ref
from conftest import GPU_ARGS, relerr
pkg = entry.load_package()
M, T, n = 64, 8, 200
g = ref.make_taps(T * M)
blk = pkg.clPolyphaseSynthesizer(*GPU_ARGS, g, M)
assert blk.route() == "generic", blk.route()
x = ref.make_input(T * M, M, M, n)
out = torch.full((n * M,), float("nan"), dtype=torch.complex64, device="cuda")
blk.work_device(n, [torch.from_numpy(x).cuda()], [out])
e = relerr(out.cpu().numpy(), ref.synth(g, M, None, x, n).astype(np.complex64))
assert e <= ref.TOL, e
print("child ok", blk.route(), e)
"""


def test_forced_generic_route_in_a_fresh_process(gpu):
    """MI355_SYNTH_GENERIC=1 is read when a handle is created: a new process (started, not exec'd over this one) gets the generic
    route at a shape the fused kernel serves here"""
    here = gpu.clPolyphaseSynthesizer(*GPU_ARGS, ref.make_taps(8 * 64), 64)
    assert here.route().startswith("fused pow2")
    here.stop()
    env = dict(os.environ, MI355_SYNTH_GENERIC="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "child ok generic" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("case,n", [((64, 8, "half"), 300), ((64, 3, "ident"), 16384 + 77), ((12, 4, "perm"), 1000), ((3, 3, "ident"), 50)], ids=str)
def test_host_pointer_general_work(gpu, case, n):
    """general_work() on numpy buffers; the second shape makes more than 2^20 outputs and is staged in two pieces"""
    M, T, kind = case
    K = T * M - 1
    m = ref.make_map(M, kind)
    nmap = ref.nmap_of(M, m)
    g = ref.make_taps(K)
    x = ref.make_input(K, M, nmap, n)
    blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g, M, m)
    y = np.full(n * M + M - 1, np.nan, np.complex64)
    assert blk.general_work(n * M + M - 1, [x.size], [x], [y]) == (n * M, n * nmap)  # whole frames only
    assert relerr(y[:n * M], ref.synth(g, M, m, x, n).astype(np.complex64)) <= ref.TOL
    assert np.all(np.isnan(y[n * M:].real))
    with pytest.raises(ValueError):
        blk.general_work(n * M, [x.size - 1], [x[:-1]], [y])
    blk.stop()


def test_set_taps_between_enqueued_calls(gpu):
    """two work_device calls on one stream with set_taps (4 -> 6 taps per arm: the history changes) between them and no
    synchronisation: the old taps entirely, then the new"""
    import torch
    M, n = 16, 40
    g1, g2 = ref.make_taps(4 * M), ref.make_taps(6 * M, seed=1)
    x1, x2 = ref.make_input(g1.size, M, M, n), ref.make_input(g2.size, M, M, n, seed=1)
    blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g1, M)
    d_x1, d_x2 = torch.from_numpy(x1).cuda(), torch.from_numpy(x2).cuda()
    o1 = torch.full((n * M,), float("nan"), dtype=torch.complex64, device="cuda")
    o2 = torch.full_like(o1, float("nan"))
    torch.cuda.synchronize()
    assert blk.work_device(n, [d_x1], [o1]) == n * M
    blk.set_taps(g2)
    assert blk.taps_per_arm() == 6
    assert blk.work_device(n, [d_x2], [o2]) == n * M
    torch.cuda.synchronize()
    assert relerr(o1.cpu().numpy(), ref.synth(g1, M, None, x1, n).astype(np.complex64)) <= ref.TOL
    assert relerr(o2.cpu().numpy(), ref.synth(g2, M, None, x2, n).astype(np.complex64)) <= ref.TOL
    blk.stop()


def test_handle_behaviour(gpu):
    import torch
    M = 64
    g1, g2 = ref.make_taps(8 * M), ref.make_taps(300 * M - 5, seed=1)
    got = []
    gpu.set_log_callback(lambda level, msg: got.append((level, msg)))
    try:
        blk = gpu.clPolyphaseSynthesizer(*GPU_ARGS, g1, M, None, 1)
    finally:
        gpu.set_log_callback(None)
    info = [msg for lvl, msg in got if lvl == 1 and msg.startswith("clPolyphaseSynthesizer:")]
    assert len(info) == 1 and "fused pow2 M=64 T=8 tile=64" in info[0] and "512 taps (8 per arm)" in info[0], got
    assert blk.history() == 7 * M and blk.num_channels() == M and blk.nmap() == M and blk.ntaps() == 8 * M
    # set_taps may change T, the history and the route
    blk.set_taps(g2)
    assert blk.taps_per_arm() == 300 and blk.history() == 299 * M and blk.route() == "generic" and np.array_equal(blk.taps(), g2)
    x = ref.make_input(g2.size, M, M, 40)
    y = _run(blk, torch.from_numpy(x).cuda(), 40, M)
    assert relerr(y, ref.synth(g2, M, None, x, 40).astype(np.complex64)) <= ref.TOL
    blk.set_taps(g1)
    assert blk.route() == "fused pow2 M=64 T=8 tile=64" and blk.history() == 7 * M
    # in == out (any overlap) is refused; nframes == 0 is a no-op; short buffers are refused before the launch
    x = ref.make_input(g1.size, M, M, 100)
    buf = torch.from_numpy(np.concatenate([x, np.zeros(100 * M, np.complex64)])).cuda()
    nin = blk.plan(100)[0]
    for src, out in ((buf, buf), (buf, buf[7:]), (buf, buf[nin - 1:]), (buf[99:], buf)):
        with pytest.raises(gpu.Mi355Error) as e:
            blk.work_device(100, [src], [out])
        assert e.value.code == -1
    assert blk.work_device(100, [buf], [buf[nin:]]) == 100 * M  # the same allocation, no overlap
    torch.cuda.synchronize()
    assert relerr(buf[nin:].cpu().numpy(), ref.synth(g1, M, None, x, 100).astype(np.complex64)) <= ref.TOL
    assert blk.work_device(0, [buf[:0]], [buf[:0]]) == 0
    assert blk.general_work(0, [0], [x[:0]], [np.empty(0, np.complex64)]) == (0, 0)
    with pytest.raises(ValueError):
        blk.work_device(100, [buf[:nin - 1]], [torch.empty(100 * M, dtype=torch.complex64, device="cuda")])
    with pytest.raises(ValueError):
        blk.work_device(100, [buf], [torch.empty(100 * M - 1, dtype=torch.complex64, device="cuda")])
    with pytest.raises(gpu.Mi355Error) as e:
        gpu.clPolyphaseSynthesizer(*GPU_ARGS, g1, M, [0, 5, 5])
    assert e.value.code == -1
    with pytest.raises(gpu.Mi355Error) as e:
        gpu.clPolyphaseSynthesizer(*GPU_ARGS, np.ones(257 * 4096, np.float32), 4096)
    assert e.value.code == -3
    blk.stop()


def _pybind():
    import glob
    import importlib.util
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block_over_uneven_pieces(gpu):
    """general_work() as the scheduler calls it: whatever input there is (history included) is offered, the block makes the whole
    frames that input and the output room allow and consumes frames x nmap; the pieces together are one synth() of the stream."""
    mod = _pybind()
    M, T = 12, 4
    K = T * M - 5
    m = ref.make_map(M, "half")
    nmap = len(m)
    g = ref.make_taps(K)
    blk = mod.clPolyphaseSynthesizer(*GPU_ARGS, g.tolist(), M, m.tolist())
    hist = (T - 1) * nmap
    assert blk.history() == hist + 1 and blk.taps_per_arm() == T and blk.nmap() == nmap and blk.num_channels() == M
    assert blk.route().startswith("fused mixed-radix") and np.array_equal(np.asarray(blk.taps(), np.float32), g)
    assert blk.forecast(10 * M + 3) == ref.plan(K, M, nmap, 10)[1]
    total = 700
    x = ref.make_input(K, M, nmap, total)
    y = np.full(total * M + 8, np.nan, np.complex64)
    rng = np.random.default_rng(4)
    pos, made = 0, 0
    for _ in range(2000):
        if made == total * M:
            break
        avail = min(int(rng.choice([hist - 1, hist, hist + nmap - 1, hist + nmap, 64, 1000])), x.size - pos)
        room = min(int(rng.choice([1, M - 1, M, 3 * M + 1, 500])), y.size - made)
        want_frames = min(max(avail - hist, 0) // nmap, room // M)
        produced, consumed = blk.general_work(room, [x[pos:pos + avail]], [y[made:made + room]])
        assert (produced, consumed) == (want_frames * M, want_frames * nmap)
        pos, made = pos + consumed, made + produced
    assert made == total * M and pos == total * nmap
    assert relerr(y[:made], ref.synth(g, M, m, x, total).astype(np.complex64)) <= ref.TOL


def test_cli_synth_only():
    r = subprocess.run([CLI, "--synth-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(rows) == 3 and all(l.startswith("clPolyphaseSynthesizer") and l.rstrip().endswith("ok") for l in rows), r.stdout
