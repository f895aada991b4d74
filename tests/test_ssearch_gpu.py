"""GPU: clSpectralSearch against tests/ssearch_ref.py.

Harmonic-sum stage (SPECTRUM input): the arithmetic is pinned, so every comparison is np.array_equal on raw bits -- the 8-byte records
and the sorted candidate set -- on both routes (route() is asserted), for pitched and misaligned buffers and for a split of the series
over handles.  Spectrum stage (SERIES input): the float32 spectrum lies within ssearch_ref.spectrum_bound of the float64 definition
(the used fraction is printed per case), bins below k_lo are +0, the bits do not depend on in_pitch, and the records equal the
yardstick's sums over the device's own spectrum bit for bit.  Every device buffer is guard-banded (tests/guarded.py) with NaN in the
gaps of a pitched input.

Shapes: Nb = 128 is one tile with blocks smaller than (16) or equal to (128) the tile; Nb = 8192 is eight tiles of 1024 bins with
blocks inside a tile (256) or spanning all of them (8192: the cross-tile atomicMax); H = 0 runs again at Nb = 1024 and 8192, where a tile
has four live waves and only the barrier in front of the key reduction orders the tile's key reset against it; N = 256, 4096, 2^17, 2^22 take the internal clFFT
through its one-pass, two-pass and four-pass routes.

On an MI355X the file takes about 6 s (66 tests); the largest used fraction of the spectrum bound is 0.109 (N = 2^17)."""
import functools
import glob
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import dedisp_ref
import fft_ref
import guarded
import psearch_ref
import ssearch_ref as ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")

SMALL = [(3, 128, Bb, H) for Bb in (16, 128) for H in range(6)]
LARGE = [(2, 8192, 256, 5), (2, 8192, 8192, 5)]
# H = 0 with four live waves per tile: no level's barrier lies between the tile's key reset and its key reduction
FLAT = [(2, 8192, 16, 0), (2, 8192, 8192, 0), (3, 1024, 16, 0), (3, 1024, 1024, 0)]
KINDS = ["exp", "integer", "constant", "inf", "negzero"]


@functools.lru_cache(maxsize=None)
def _w(S, Nb, kind):
    rng = np.random.default_rng(100 + S + Nb + len(kind))
    if kind == "exp":
        w = rng.exponential(1.0, (S, Nb))
    elif kind == "integer":
        w = rng.integers(0, 9, (S, Nb))
    elif kind == "constant":
        w = np.ones((S, Nb))
    elif kind == "inf":
        w = rng.exponential(1.0, (S, Nb))
        w[0, Nb // 3] = np.inf
        w[S - 1, 5] = -np.inf
        w[S - 1, Nb - 2] = np.inf   # +Inf and -Inf meet in the sums of series S - 1: NaN where the formula gives it
    elif kind == "negzero":
        w = np.zeros((S, Nb))
        w[:, 1::2] = -0.0
        w[0, Nb // 2:] = rng.exponential(1.0, Nb - Nb // 2) - 1.0
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _want(S, Nb, Bb, H, kind):
    pk = ref.peaks(_w(S, Nb, kind), H, Bb)
    pk.setflags(write=False)
    return pk


def _block(pkg, S, Nb, Bb, H, generic, max_cands=0, kind=ref.SPECTRUM, k_lo=1, inv_sigma=None):
    blk = pkg.clSpectralSearch(*GPU_ARGS, S, 2 * Nb, H, Bb, k_lo, kind, inv_sigma, max_cands)
    blk.set_generic(generic)
    head = "%s S=%d N=%d H=%d Bb=%d" % ("generic" if generic else "tiled", S, 2 * Nb, H, Bb)
    tail = " spectrum" if kind == ref.SPECTRUM else " series k_lo=%d" % k_lo
    assert blk.route().startswith(head + ("" if generic else " tk=%d" % min(Nb, 1024)) + tail), blk.route()
    return blk


def _run(blk, x, pitch=None, in_off=0, peaks_off=0, spectrum=False, spec_off=0):
    """work_device on guard-banded buffers; x[S][row].  Returns (peaks [S][nblk], spectrum [S][Nb] or None, sorted candidates or None,
    found)"""
    import torch
    S, row, Nb = blk.num_series, blk.row, blk.num_bins
    buf = ref.pitched(x, row if pitch is None else pitch)
    wi, vi = guarded.guarded_input(buf, guarded.pad_items(4, row), in_off, "cuda")
    wo, vo = guarded.guarded_output(2 * S * blk.records, np.float32, guarded.pad_items(4, 2 * blk.records), peaks_off, "cuda")
    outs = [vo]
    if spectrum:
        ws, vs = guarded.guarded_output(S * Nb, np.float32, guarded.pad_items(4, Nb), spec_off, "cuda")
        outs.append(vs)
    cands = counts = None
    if blk.max_cands:
        wc, cands = guarded.guarded_output(4 * blk.max_cands, np.int32, guarded.pad_items(4, 64), 2, "cuda")
        wn, counts = guarded.guarded_output(2, np.int32, guarded.pad_items(4, 64), 2, "cuda")
    assert blk.work_device([vi], outs, pitch, cands, counts) == 1
    torch.cuda.synchronize()
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "peaks", interior=False)
    pk = blk.peaks_of(vo).reshape(S, blk.records)
    assert not (pk["loc"] == guarded.NAN_BITS).any(), "a record was not written"
    spec = None
    if spectrum:
        guarded.check_guards(ws, vs, "spectrum", interior=False)
        spec = guarded.to_numpy(vs).reshape(S, Nb)
    got = found = None
    if blk.max_cands:
        guarded.check_guards(wc, cands, "cands", interior=False)
        guarded.check_guards(wn, counts, "counts", interior=False)
        rec, found = blk.candidates()
        got = psearch_ref.sort_records(rec)
    return pk, spec, got, found


def _same(pk, want):
    assert np.array_equal(pk.view(np.uint64), want.view(np.uint64)), np.argwhere(pk.view(np.uint64) != want.view(np.uint64))[:4]
    return True


@pytest.mark.parametrize("generic", [False, True], ids=["tiled", "generic"])
@pytest.mark.parametrize("shape", SMALL + LARGE + FLAT, ids=lambda s: "S%d_Nb%d_Bb%d_H%d" % s)
def test_sums_equal_the_reference(gpu, pkg, shape, generic):
    """every input kind, each also at in_pitch = Nb + 3 with `in` one float past a 16-byte boundary and the peaks at an 8-byte boundary
    that is not a 16-byte one"""
    S, Nb, Bb, H = shape
    blk = _block(pkg, S, Nb, Bb, H, generic)
    for kind in KINDS:
        want = _want(S, Nb, Bb, H, kind)
        if kind == "constant":
            assert (want["loc"] == 0).all() and (want["snr"].view(np.uint32) == 0).all()  # every tie goes to h = 0 and the smallest k
        assert _same(_run(blk, _w(S, Nb, kind))[0], want)
        assert _same(_run(blk, _w(S, Nb, kind), pitch=Nb + 3, in_off=1, peaks_off=2)[0], want)


def _reads(Nb, H, m):
    """the (h, k) whose sum reads bin m, literally"""
    out = np.zeros((H + 1, Nb), bool)
    for h in range(H + 1):
        for k in range(Nb):
            out[h, k] = k == m or any(ref.r(k, j, hh) == m for hh in range(1, h + 1) for j in range(1, 1 << hh, 2))
    return out


@pytest.mark.parametrize("generic", [False, True], ids=["tiled", "generic"])
@pytest.mark.parametrize("shape", [(3, 128, 16, 5), (3, 128, 128, 5), (2, 8192, 256, 5), (2, 8192, 8192, 5)], ids=lambda s: "S%d_Nb%d_Bb%d_H%d" % s)
def test_single_nans_remove_what_the_formula_gives(gpu, pkg, shape, generic):
    """one NaN at m = 0, at a tile's first and last bin and at Nb - 1, in one series: the yardstick's NaN set is exactly the (h, k) whose
    sum reads m (checked literally at Nb = 128), the other series keep their bits, and the device equals the yardstick"""
    S, Nb, Bb, H = shape
    blk = _block(pkg, S, Nb, Bb, H, generic)
    clean = _want(S, Nb, Bb, H, "exp")
    for i, m in enumerate(sorted({0, min(Nb, 1024) - 1, min(Nb, 1024) % Nb, Nb - 1})):
        s = i % S
        w = np.array(_w(S, Nb, "exp"))
        w[s, m] = np.nan
        if Nb == 128:
            assert np.array_equal(np.isnan(ref.snr(w, H)[:, s]), _reads(Nb, H, m))
        want = ref.peaks(w, H, Bb)
        others = [t for t in range(S) if t != s]
        assert np.array_equal(want[others].view(np.uint64), clean[others].view(np.uint64))
        assert _same(_run(blk, w, pitch=Nb + 3, in_off=1)[0], want)
    pk = _run(blk, np.full((S, Nb), np.nan, np.float32))[0]
    assert (pk["loc"] == 0xFFFFFFFF).all() and np.isneginf(pk["snr"]).all()


@pytest.mark.parametrize("generic", [False, True], ids=["tiled", "generic"])
@pytest.mark.parametrize("shape", [(3, 128, 16, 5), (2, 8192, 256, 5)], ids=lambda s: "S%d_Nb%d_Bb%d_H%d" % s)
def test_candidates(gpu, pkg, shape, generic):
    """the thresholded list is the yardstick's set; a capacity below the number found gives a subset and counts = (found, capacity)"""
    S, Nb, Bb, H = shape
    want = _want(S, Nb, Bb, H, "exp")
    thr = float(np.sort(want["snr"].reshape(-1))[want.size // 2])
    cset = ref.candidates(want, thr)
    assert 2 <= len(cset) < want.size
    blk = _block(pkg, S, Nb, Bb, H, generic, max_cands=want.size)
    pk, _, got, found = _run(blk, _w(S, Nb, "exp"))
    assert _same(pk, want) and found == 0 and len(got) == 0  # the threshold is +Inf at first
    blk.set_threshold(thr)
    pk, _, got, found = _run(blk, _w(S, Nb, "exp"), pitch=Nb + 3, in_off=1, peaks_off=2)
    assert _same(pk, want) and found == len(cset) and np.array_equal(got, cset)
    with pytest.raises(pkg.Mi355Error):
        blk.set_threshold(float("nan"))
    cap = len(cset) // 2
    small = _block(pkg, S, Nb, Bb, H, generic, max_cands=cap)
    small.set_threshold(thr)
    pk, _, got, found = _run(small, _w(S, Nb, "exp"))
    assert _same(pk, want) and found == len(cset) and len(got) == cap
    assert set(map(tuple, got)) <= set(map(tuple, cset))


@pytest.mark.parametrize("generic", [False, True], ids=["tiled", "generic"])
def test_series_split_over_calls(gpu, pkg, generic):
    """S = 3 as 1 + 2: the same record bits and the same candidate set (series counted from each call's first)"""
    S, Nb, Bb, H = 3, 128, 16, 5
    w, want = _w(S, Nb, "exp"), _want(S, Nb, Bb, H, "exp")
    thr = float(np.sort(want["snr"].reshape(-1))[want.size // 2])
    parts = []
    for s0, ns in ((0, 1), (1, 2)):
        blk = _block(pkg, ns, Nb, Bb, H, generic, max_cands=want.size)
        blk.set_threshold(thr)
        pk, _, got, _ = _run(blk, w[s0:s0 + ns], pitch=Nb + 3, in_off=1)
        assert _same(pk, want[s0:s0 + ns])
        got = got.copy()
        got[:, 2] += s0
        parts.append(got)
    assert np.array_equal(psearch_ref.sort_records(np.concatenate(parts)), ref.candidates(want, thr))


def test_tiled_equals_generic_on_a_long_spectrum(gpu, pkg):
    """Nb = 2^16, 64 tiles per series, without the yardstick: the two routes agree bit for bit"""
    S, Nb, Bb, H = 2, 1 << 16, 4096, 5
    w = np.random.default_rng(3).exponential(1.0, (S, Nb)).astype(np.float32)
    a = _run(_block(pkg, S, Nb, Bb, H, False), w, pitch=Nb + 1, in_off=3)[0]
    b = _run(_block(pkg, S, Nb, Bb, H, True), w)[0]
    assert _same(a, b)


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    S, Nb = 3, 128
    blk = _block(pkg, S, Nb, 16, 5, False, max_cands=4)
    ser = _block(pkg, S, Nb, 16, 5, False, kind=ref.SERIES)
    x = torch.zeros(S * 2 * Nb + 8, dtype=torch.float32, device="cuda")
    outs = [guarded.guarded_output(m, np.float32, guarded.pad_items(4, 64), 0, "cuda") for m in (2 * S * blk.records + 8, S * Nb + 8, 16 + 8, 2 + 8)]
    (wy, y), (wz, z), (wc, c), (wn, n) = outs   # peaks, spectrum, cands, counts: guard-banded, NaN bit patterns inside
    L, vp = pkg.lib(), lambda t, off=0: t.data_ptr() + off
    #        in        pitch     peaks      spectrum  cands  max counts
    bad = [(None, Nb, vp(y), None, None, 0, None), (vp(x), Nb, None, None, None, 0, None), (vp(x, 2), Nb, vp(y), None, None, 0, None),
           (vp(x), Nb, vp(y, 4), None, None, 0, None), (vp(x), Nb - 1, vp(y), None, None, 0, None), (vp(x), Nb, vp(x), None, None, 0, None),
           (vp(x), Nb, vp(y), vp(z), None, 0, None),                      # a spectrum output with SPECTRUM input
           (vp(x), Nb, vp(y), None, vp(c), 4, None),                      # cands without counts
           (vp(x), Nb, vp(y), None, vp(c, 4), 4, vp(n)), (vp(x), Nb, vp(y), None, vp(c), 4, vp(n, 4)), (vp(x), Nb, vp(y), None, vp(c), -1, vp(n)),
           (vp(x), Nb, vp(y), None, vp(y, 16), 4, vp(n)), (vp(x), Nb, vp(y), None, vp(c), 4, vp(c, 8)), (vp(x), Nb, vp(y), None, vp(x, 64), 4, vp(n)),
           (vp(x), (1 << 38) // S + 1, vp(y), None, None, 0, None)]
    for a in bad:
        rc = L.mi355_ssearch_work_dev(blk._h, *a, None)
        assert rc == (-3 if a[1] > 1 << 30 else -1), (a, L.mi355_last_error().decode())
    N = 2 * Nb
    for a in [(vp(x, 4), N, vp(y), vp(z), None, 0, None), (vp(x), N + 1, vp(y), vp(z), None, 0, None), (vp(x), N - 2, vp(y), vp(z), None, 0, None),
              (vp(x), N, vp(y), vp(z, 2), None, 0, None), (vp(x), N, vp(y), vp(x, 64), None, 0, None), (vp(x), N, vp(y), vp(y, 32), None, 0, None)]:
        assert L.mi355_ssearch_work_dev(ser._h, *a, None) == -1, (a, L.mi355_last_error().decode())
    torch.cuda.synchronize()
    for whole, view in outs:
        guarded.check_guards(whole, view, "output of a refused call", interior=False)
        assert (view.view(torch.int32) == guarded.NAN_BITS).all(), "a refused call wrote"
    with pytest.raises(ValueError):
        blk.work_device([x[:S * Nb - 1]], [y])


# ---- spectrum stage ----

@functools.lru_cache(maxsize=None)
def _cases(N):
    out = ref.series_cases(N)
    for x, g in out.values():
        x.setflags(write=False)
    return out


@pytest.mark.parametrize("case", ["tones", "scaled"])
@pytest.mark.parametrize("N", [256, 4096, 1 << 17, 1 << 22], ids=lambda n: "N%d" % n)
def test_spectrum_within_the_bound_and_records_of_its_own_spectrum(gpu, pkg, N, case):
    x, g = _cases(N)[case]
    S, Nb, Bb, H, k_lo = x.shape[0], N // 2, 64, 5, 3
    blk = _block(pkg, S, Nb, Bb, H, False, kind=ref.SERIES, k_lo=k_lo, inv_sigma=g)
    pk, spec, _, _ = _run(blk, x, spectrum=True)
    route = blk.fft_route()
    assert route.startswith({256: "k_fft<128>", 4096: "k_fft<2048>", 1 << 17: "k_fft_tile ", 1 << 22: "k_fft_sub+combine2 "}[N]), route
    used = ref.spectrum_used(spec, x, g, k_lo, fft_ref.fft_bound_kind(route))
    print("N = %d, %s: the spectrum uses %.4f of its bound (%s)" % (N, case, used, route))
    assert used <= 1.0
    assert (spec[:, :k_lo].view(np.uint32) == 0).all()
    if case == "scaled":
        assert (spec[0].view(np.uint32) == 0).all()  # a series of zeros: exactly +0
    if case == "tones" and N == 1 << 17:
        assert 0.9 <= spec[0].mean() <= 1.1
    # the records are the yardstick's sums over the device's own spectrum (the first series alone at the longest length)
    sel = slice(0, 1) if N == 1 << 22 and case == "tones" else slice(0, S)
    want = ref.peaks(spec[sel], H, Bb)
    assert _same(pk[sel], want)
    # in_pitch = N + 2 (packed through scratch), `in` 8-byte but not 16-byte aligned, no spectrum output, the generic route
    pk2, spec2, _, _ = _run(blk, x, pitch=N + 2, in_off=2, peaks_off=2, spectrum=True, spec_off=1)
    assert np.array_equal(spec2.view(np.uint32), spec.view(np.uint32)) and np.array_equal(pk2.view(np.uint64), pk.view(np.uint64))
    blk.set_generic(True)
    assert np.array_equal(_run(blk, x, in_off=2)[0].view(np.uint64), pk.view(np.uint64))


def test_alignment_of_the_16_byte_transforms(gpu, pkg):
    """Nb = 8192 and 16384 are the lengths whose clFFT kernel reads 16 bytes per lane (clFFT asks for a 16-byte boundary above 4096
    points): an input at an 8-byte boundary that is not a 16-byte one goes through scratch and gives the same bits"""
    for N in (16384, 32768):
        x, g = _cases(N)["tones"]
        blk = _block(pkg, 3, N // 2, 256, 5, False, kind=ref.SERIES, k_lo=2, inv_sigma=g)
        pk, spec, _, _ = _run(blk, x, spectrum=True)
        assert ref.spectrum_used(spec, x, g, 2, fft_ref.fft_bound_kind(blk.fft_route())) <= 1.0
        pk2, spec2, _, _ = _run(blk, x, in_off=2, spectrum=True)
        assert np.array_equal(spec2.view(np.uint32), spec.view(np.uint32)) and np.array_equal(pk2.view(np.uint64), pk.view(np.uint64))


def test_series_split_and_set_stats(gpu, pkg):
    """SERIES input: the spectrum bits of a series do not depend on which other series share the call; a call after set_stats uses the
    new inv_sigma entirely"""
    N = 4096
    x, g = _cases(N)["tones"]
    blk = _block(pkg, 3, N // 2, 64, 5, False, kind=ref.SERIES, k_lo=3, inv_sigma=g)
    pk, spec, _, _ = _run(blk, x, spectrum=True)
    for s0, ns in ((0, 1), (1, 2)):
        part = _block(pkg, ns, N // 2, 64, 5, False, kind=ref.SERIES, k_lo=3, inv_sigma=g[s0:s0 + ns])
        pk1, spec1, _, _ = _run(part, x[s0:s0 + ns], spectrum=True)
        assert np.array_equal(spec1.view(np.uint32), spec[s0:s0 + ns].view(np.uint32)) and _same(pk1, pk[s0:s0 + ns])
    ones = _block(pkg, 3, N // 2, 64, 5, False, kind=ref.SERIES, k_lo=3)
    assert np.array_equal(ones.stats(), np.ones(3, np.float32))
    ones.set_stats(g)
    assert np.array_equal(ones.stats(), g)
    pk3, spec3, _, _ = _run(ones, x, spectrum=True)
    assert np.array_equal(spec3.view(np.uint32), spec.view(np.uint32)) and _same(pk3, pk)
    with pytest.raises(ValueError):
        ones.set_stats(np.ones(2, np.float32))


def test_host_work_in_pieces(gpu, pkg):
    """work() on numpy buffers: a series of 2^20 samples is a staged piece of its own, so the two series go one by one, each with its
    own inv_sigma, and the candidates of the second piece carry series 1; everything equals the device path bit for bit"""
    N, S, Bb, H = 1 << 20, 2, 1024, 5
    rng = np.random.default_rng(21)
    x = np.stack([ref.pulse_train(rng, N, 12.8, 1.0), (3 * rng.standard_normal(N)).astype(np.float32)])
    g = psearch_ref.measure(x, N)[1].astype(np.float32)
    blk = _block(pkg, S, N // 2, Bb, H, False, max_cands=S * N // 2 // Bb, kind=ref.SERIES, k_lo=4, inv_sigma=g)
    blk.set_threshold(8.0)
    pk, spec, cands, found = _run(blk, x, spectrum=True)
    assert found >= 2 and len(set(cands[:, 2])) == 2, "the case is meant to list candidates of both series"
    buf = ref.pitched(x, N + 6)
    for generic in (False, True):
        blk.set_generic(generic)
        hpk, hspec = blk.search(buf, N + 6, spectrum=True)
        rec, hfound = blk.candidates()
        assert _same(hpk, pk) and np.array_equal(hspec.view(np.uint32), spec.view(np.uint32))
        assert hfound == found and np.array_equal(psearch_ref.sort_records(rec), cands)
    assert blk.best(hpk) == ref.best(pk, Bb) + (float(pk["snr"].max()),)
    s, h, k, snr = blk.best(hpk)
    assert (s, h, k) == (0, 2, 4 * N // 128 * 10)  # the fundamental lies on bin N / 12.8; level 2 holds harmonics 1 .. 4 of the six


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu, pkg):
    """the C++ block as the scheduler calls it: work() on numpy buffers, two segments in, two items of records and spectra out, equal
    to the ctypes block's device path bit for bit"""
    mod = _pybind()
    N = 4096
    x, g = _cases(N)["tones"]
    pk, spec, _, _ = _run(_block(pkg, 3, N // 2, 64, 5, False, kind=ref.SERIES, k_lo=3, inv_sigma=g), x, spectrum=True)
    ss = mod.clSpectralSearch(*GPU_ARGS, 3, N, 5, 64, 3, g)
    assert ss.history() == 1 and ss.segment_len() == N and ss.num_bins() == N // 2 and ss.records_per_series() == 32
    assert ss.freq(2, 1280, 1e-3) == pkg.ssearch_freq(N, 1e-3, 2, 1280) and np.array_equal(ss.inv_sigma(), g)
    two = np.concatenate([x.reshape(-1), x.reshape(-1)])
    for generic in (False, True):
        ss.set_generic(generic)
        assert ss.route().startswith("generic " if generic else "tiled ")
        y = np.zeros((2,) + pk.shape, ref.PEAK)
        w = np.full((2,) + spec.shape, np.nan, np.float32)
        assert ss.work(2, [two], [y, w]) == 2
        for item in range(2):
            assert _same(y[item], pk) and np.array_equal(w[item].view(np.uint32), spec.view(np.uint32))
        y[:] = 0
        assert ss.work(1, [x], [y[:1]]) == 1 and _same(y[0], pk)
    with pytest.raises(ValueError):
        ss.set_stats(np.zeros(2, np.float32))
    with pytest.raises(ValueError):
        ss.work(1, [x.reshape(-1)[:-1]], [y])  # one float fewer than the call reads
    with pytest.raises(ValueError):
        mod.clSpectralSearch(*GPU_ARGS, 3, N, 6, 64)


def test_cli_row(gpu):
    """test-clenabled-mi355 --ssearch-only runs the smallest shape on generated samples, prints its spectrum and the checksum of its
    records and exits 0: the spectrum lies within the bound and the records are the yardstick's sums over it"""
    r = subprocess.run([CLI, "--ssearch-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    state, vals = 12345, np.empty(256, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    x = (vals + 1).astype(np.float32)[None]
    g = np.array([1.0 / 64.0], np.float32)
    w = np.array([int(v, 16) for l in r.stdout.splitlines() if l.startswith("w ") for v in l.split()[1:]], np.uint32).view(np.float32)[None]
    assert w.shape == (1, 128) and ref.spectrum_used(w, x, g, 1) <= 1.0
    pk = ref.peaks(w, 5, 16)
    u = np.uint64

    def wsum(a, mod):
        a = a.reshape(-1).astype(u)
        return int(((np.arange(a.size, dtype=u) % u(mod) + u(1)) * a).sum(dtype=u))

    want = (wsum(pk["snr"].view(np.uint32), 7) + wsum(pk["loc"], 7)) % (1 << 64)
    m = re.search(r"^clSpectralSearch checksum (\d+) spectrum (\d+)$", r.stdout, re.M)
    assert m.group(1) == str(want) and m.group(2) == str(wsum(w.view(np.uint32), 5)), r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clSpectralSearch (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout


def test_dedisperser_feeds_the_search_and_the_search_the_folder(gpu, pkg):
    """F = 64 channels, D = 4 trials, N = 4096: a filterbank with a dispersed train of one-sample pulses every 12.8 samples (below the
    FFA's floor) -> clDedisperser (per-trial output) -> measure -> clSpectralSearch, all on the device: the best record lies at the
    injected trial, level 2, bin 1280; mi355_ssearch_freq gives the period mi355_fold_model takes, and clFolder's profile of the channel
    without delay peaks in the bin that holds the pulses"""
    import torch
    F, D, N, d_true, tsamp, period = 64, 4, 4096, 2, 1e-3, 12.8
    delay = np.rint(np.arange(D)[:, None] * 12.0 * (F - 1 - np.arange(F))[None, :] / (F - 1)).astype(np.int32)
    Hd = int(delay.max())
    rng = np.random.default_rng(11)
    x = rng.normal(1.0, 0.25, (N + Hd, 1, F)).astype(np.float32)   # the sum over the band: mean 64, sigma 2
    t = np.arange(N + Hd)
    for f in range(F):
        x[:, 0, f] += np.float32(12.0 / F) * (((t - delay[d_true, f] + 0.5) % period) < 1.0)   # 6 sigma of the sum
    dd = pkg.clDedisperser(*GPU_ARGS, 1, F, D, Hd, pkg.DEDISP_TRIAL_MAJOR, delay)
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    w_series, d_series = guarded.guarded_output(D * N, np.float32, guarded.pad_items(4, N), 0, "cuda")
    assert dd.work_device(N, [d_x], [d_series]) == N
    torch.cuda.synchronize()
    guarded.check_guards(w_series, d_series, "series")
    series = dedisp_ref.dedisperse(x, delay, N, dedisp_ref.TRIAL_MAJOR).reshape(D, N)
    assert np.array_equal(d_series.cpu().numpy().view(np.uint32), series.reshape(-1).view(np.uint32))
    mean, isg = pkg.clPulseSearch(*GPU_ARGS, 1, D, 1, 16, pkg.PSEARCH_TRIAL_MAJOR).measure(d_series, N)
    assert np.allclose(isg, psearch_ref.measure(series, N)[1], rtol=1e-6)
    blk = pkg.clSpectralSearch(*GPU_ARGS, D, N, 5, 16, 2, pkg.SSEARCH_SERIES, isg)
    for generic in (False, True):
        blk.set_generic(generic)
        w_pk, d_pk = guarded.guarded_output(2 * D * blk.records, np.float32, guarded.pad_items(4, 2 * blk.records), 0, "cuda")
        w_spec, d_spec = guarded.guarded_output(D * blk.num_bins, np.float32, guarded.pad_items(4, blk.num_bins), 0, "cuda")
        assert blk.work_device([d_series], [d_pk, d_spec]) == 1
        torch.cuda.synchronize()
        guarded.check_guards(w_pk, d_pk, "peaks", interior=False)
        guarded.check_guards(w_spec, d_spec, "spectrum")
        pk = blk.peaks_of(d_pk).reshape(D, blk.records)
        assert _same(pk, ref.peaks(d_spec.cpu().numpy().reshape(D, -1), 5, 16))
        s, h, k, snr = blk.best(pk)
        assert (s, h, k) == (d_true, 2, 1280) and snr > 1.3 * np.delete(pk["snr"].max(axis=1), d_true).max()
    p_s = 1.0 / pkg.ssearch_freq(N, tsamp, h, k)
    assert abs(p_s - period * tsamp) < 1e-15
    nbin, Ts = 8, 64
    model = pkg.fold_model(p_s, 0.0, tsamp, 0.5 / nbin).reshape(1, 3)   # the pulses, within half a sample of phase 0, sit inside bin 0
    fo = pkg.clFolder(*GPU_ARGS, 1, F, nbin, Ts, model)
    ns = N // Ts
    w_out, d_out = guarded.guarded_output(ns * nbin * F, np.float32, guarded.pad_items(4, nbin * F), 0, "cuda")
    assert fo.work_device(ns, [d_x], [d_out]) == ns
    torch.cuda.synchronize()
    guarded.check_guards(w_out, d_out, "archive")
    prof = d_out.cpu().numpy().reshape(ns, nbin, F).astype(np.float64).sum(axis=0)[:, F - 1]   # the channel whose delay is 0 at every trial
    assert int(np.argmax(prof)) == 0 and prof[0] - np.median(prof) > 5 * 0.25 * np.sqrt(N / nbin)
