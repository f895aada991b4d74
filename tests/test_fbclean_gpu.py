"""GPU: clFilterbankCleaner against tests/fbclean_ref.py (numpy: the contract's segment sums and tree in float64, the flag, the two-rounding
float32 normalisation, the 64-partial zero-DM sum).  The arithmetic is pinned, so every comparison is np.array_equal on the raw bits of
`out` and `stats` and on the flag bytes.  Every device call runs on guard-banded buffers (tests/guarded.py); `out` and `stats` hold NaN
bit patterns and the flag buffers 0xFF before the call, so an item the call never wrote shows.

Routes, as csrc/fbclean.hip and the header state them:
  slab     F a multiple of 256 in 256 .. 4096, every Tb: k_fb_slab, one workgroup per (block, row)
  generic  every other shape and every handle under set_generic(True): k_fb_stat / k_fb_zdm / k_fb_apply
Every test asserts the route it expects through route().

Shapes stay small: the largest input is (2, 256, 4096, 1), 8 MiB."""
import ctypes as C
import functools
import glob
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GPU_ARGS, ROOT
import beamform_ref
import dedisp_ref
import fbclean_ref as ref
import guarded
import psearch_ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
INF = float("inf")

# (R, F, Tb, blocks)
SLAB = [(3, 256, 32, 3),     # one channel group, segments of 2
        (2, 512, 48, 2),     # two groups, odd segment length
        (1, 4096, 64, 1),    # the widest band
        (2, 256, 4096, 1),   # the longest block
        (64, 256, 32, 1)]    # many slabs
GENERIC = [(3, 52, 48, 2), (1, 5, 16, 3), (2, 260, 32, 1)]
KINDS = ["gamma", "wide", "nan", "nanrun", "inf", "const", "masked", "nozdm", "nolimits"]


def _limits(kind, Tb):
    """(nd, sk_lo, sk_hi, td, zero_dm): limits that flag some cells of the gamma fixture and leave most"""
    w = 1.5 * 2.0 / np.sqrt(Tb)
    if kind == "wide":
        return (1.0, -INF, INF, 2.0, 1)  # the spectral kurtosis of exp2(uniform) data would flag everything
    if kind == "nolimits":
        return (16.0, -INF, INF, INF, 1)
    return (16.0, 1.0 - w, 1.0 + w, 2.0, 0 if kind == "nozdm" else 1)


@functools.lru_cache(maxsize=None)
def _case(kind, R, F, Tb, nb):
    """(x[n][R][F] float32 read-only, mask[F] uint8)"""
    rng = np.random.default_rng(7000 + R * 3 + F * 5 + Tb * 7 + nb + len(kind))
    n = nb * Tb
    x = ref.wide_range(rng, n, R, F) if kind == "wide" else ref.gamma(rng, n, R, F)
    mask = np.zeros(F, np.uint8)
    mask[F // 3] = 1
    mask[F - 1] = 7
    r, f = R // 2, F // 2
    if kind == "nan":
        x[n // 3, r, f] = np.nan
    elif kind == "nanrun":  # across the first block boundary where there is one
        x[max(Tb - 3, 0):Tb + 4, r, f] = np.nan
        x[5, 0, 0] = np.nan
    elif kind == "inf":
        x[7, 0, 1] = np.inf
        x[n - 1, R - 1, F - 2] = -np.inf
        x[n // 2, r, f] = np.inf
        x[n // 2 + 1, r, f] = -np.inf
    elif kind == "const":
        x[:, r, f] = np.float32(3.25)          # the whole column
        x[:Tb, 0, 2] = np.float32(-1.5)        # one block only
        x[:, R - 1, 3] = 0.0
    elif kind == "masked":
        mask[:] = 1
    x.setflags(write=False)
    mask.setflags(write=False)
    return x, mask


@functools.lru_cache(maxsize=None)
def _want(kind, R, F, Tb, nb):
    x, mask = _case(kind, R, F, Tb, nb)
    res = ref.clean(x, Tb, *_limits(kind, Tb), mask=mask)
    for a in res:
        a.setflags(write=False)
    return res


def _block(pkg, kind, R, F, Tb, nb=1):
    return pkg.clFilterbankCleaner(*GPU_ARGS, R, F, Tb, *_limits(kind, Tb), mask=_case(kind, R, F, Tb, nb)[1])


def _run(blk, x, in_off=0, out_off=0, in_place=False, opt=(True, True, True)):
    """work_device on guard-banded buffers; x[n][R][F].  Returns (out, cflags, tflags, stats), None for an output that was not asked for"""
    import torch
    n, R, F = x.shape
    nb = n // blk.block_len
    wi, vi = guarded.guarded_input(x, guarded.pad_items(4, R * F), in_off, "cuda")
    if in_place:
        wo, vo = wi, vi
    else:
        wo, vo = guarded.guarded_output(x.size, np.float32, guarded.pad_items(4, R * F), out_off, "cuda")
    bufs = [None, None, None]
    if opt[0]:
        bufs[0] = guarded.guarded_output(nb * R * F, np.int8, guarded.pad_items(1, R * F), 0, "cuda")
    if opt[1]:
        bufs[1] = guarded.guarded_output(n * R, np.int8, guarded.pad_items(1, R), 0, "cuda")
    if opt[2]:
        bufs[2] = guarded.guarded_output(2 * nb * R * F, np.float32, guarded.pad_items(4, 2 * R * F), 0, "cuda")
    for b in bufs[:2]:
        if b is not None:
            b[1].fill_(-1)  # 0xFF: neither 0 nor 1
    assert blk.work_device(n, [vi], [vo] + [None if b is None else b[1] for b in bufs]) == n
    torch.cuda.synchronize()
    guarded.check_guards(wi, vi, "input")
    if not in_place:
        guarded.check_guards(wo, vo, "out")
    names = ("cflags", "tflags", "stats")
    got = [guarded.to_numpy(vo).reshape(n, R, F)]
    for k, b in enumerate(bufs):
        if b is None:
            got.append(None)
            continue
        guarded.check_guards(b[0], b[1], names[k], interior=(k == 2))
        got.append(guarded.to_numpy(b[1]))
    if got[1] is not None:
        got[1] = got[1].view(np.uint8).reshape(nb, R, F)
    if got[2] is not None:
        got[2] = got[2].view(np.uint8).reshape(n, R)
    if got[3] is not None:
        got[3] = got[3].reshape(nb, R, F, 2)
    return tuple(got)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want):
    """every output that was asked for, bit for bit"""
    return all(g is None or (g.shape == w.shape and np.array_equal(_bits(g), _bits(w))) for g, w in zip(got, want))


def _route_of(F):
    return "slab" if F % 256 == 0 and F <= 4096 else "generic"


def _both_routes(blk, expect_route):
    """yields the route names after asserting them: the geometry's own route, then the forced generic one"""
    assert blk.route().startswith(expect_route + " "), blk.route()
    yield blk.route()
    blk.set_generic(True)
    assert blk.route().startswith("generic "), blk.route()
    yield blk.route()
    blk.set_generic(False)
    assert blk.route().startswith(expect_route + " ")


def test_route_names_its_plan(gpu, pkg):
    assert pkg.clFilterbankCleaner(*GPU_ARGS, 64, 1024, 256).route() == "slab R=64 F=1024 Tb=256 fg=256"
    assert pkg.clFilterbankCleaner(*GPU_ARGS, 3, 52, 48).route() == "generic R=3 F=52 Tb=48"
    for R, F, Tb, nb in SLAB:
        assert pkg.clFilterbankCleaner(*GPU_ARGS, R, F, Tb).route() == "slab R=%d F=%d Tb=%d fg=256" % (R, F, Tb)
    for R, F, Tb, nb in GENERIC + [(2, 4352, 16, 1), (1, 128, 32, 1)]:
        assert pkg.clFilterbankCleaner(*GPU_ARGS, R, F, Tb).route() == "generic R=%d F=%d Tb=%d" % (R, F, Tb)
    blk = pkg.clFilterbankCleaner(*GPU_ARGS, 2, 256, 32, 16.0, 0.5, 1.5, 3.0, 1)
    assert blk.limits() == (16.0, 0.5, 1.5, 3.0, 1) and not blk.mask().any() and blk.floats_per_sample() == 512
    assert pkg.lib().mi355_fbclean_block_len(blk._h) == 32


@pytest.mark.parametrize("R,F,Tb,nb", SLAB + GENERIC)
def test_shapes(gpu, pkg, R, F, Tb, nb):
    """every slab shape on the slab route and again on the generic one (slab == generic == reference), every generic shape"""
    x, mask = _case("gamma", R, F, Tb, nb)
    want = _want("gamma", R, F, Tb, nb)
    assert 0 < want[1].mean() < 0.6 and (want[2].any() or nb * Tb * R < 100)  # the fixture exercises both flags
    blk = _block(pkg, "gamma", R, F, Tb, nb)
    for r in _both_routes(blk, _route_of(F)):
        assert _same(_run(blk, x), want), r


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,F,Tb,nb", [(2, 512, 48, 2), (3, 52, 48, 2)])
def test_data_sets(gpu, pkg, kind, R, F, Tb, nb):
    x, mask = _case(kind, R, F, Tb, nb)
    want = _want(kind, R, F, Tb, nb)
    if kind in ("nan", "nanrun", "inf", "const"):  # the bad cells are flagged, carry {0, 0}, and reach nothing else
        assert want[1][:, R // 2, F // 2].any() and not np.isnan(want[0]).any() and np.isfinite(want[3]).all()
    if kind == "masked":
        assert want[1].all() and not want[0].any() and not want[2].any() and want[3].any()
    if kind == "nozdm":
        assert not want[2].any()
    blk = _block(pkg, kind, R, F, Tb, nb)
    for r in _both_routes(blk, _route_of(F)):
        assert _same(_run(blk, x), want), r


@pytest.mark.parametrize("R,F,Tb", [(3, 256, 32), (3, 52, 48)])
def test_every_split_of_three_blocks(gpu, pkg, R, F, Tb):
    x, mask = _case("gamma", R, F, Tb, 3)
    want = _want("gamma", R, F, Tb, 3)
    blk = _block(pkg, "gamma", R, F, Tb, 3)
    for r in _both_routes(blk, _route_of(F)):
        for split in ((3,), (1, 2), (2, 1), (1, 1, 1)):
            parts, b0 = [], 0
            for nb in split:
                parts.append(_run(blk, x[b0 * Tb:(b0 + nb) * Tb]))
                b0 += nb
            got = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
            assert _same(got, want), (r, split)


@pytest.mark.parametrize("R,F,Tb,nb", [(2, 512, 48, 2), (2, 260, 32, 1)])
def test_alignment_and_in_place(gpu, pkg, R, F, Tb, nb):
    """in / out one float (and three, and two) past a 16-byte boundary; out == in equals out of place"""
    x, mask = _case("gamma", R, F, Tb, nb)
    want = _want("gamma", R, F, Tb, nb)
    blk = _block(pkg, "gamma", R, F, Tb, nb)
    for r in _both_routes(blk, _route_of(F)):
        for in_off, out_off in ((1, 0), (0, 1), (1, 1), (3, 2)):
            assert _same(_run(blk, x, in_off, out_off), want), (r, in_off, out_off)
        for off in (0, 1):
            assert _same(_run(blk, x, off, in_place=True), want), (r, off)


@pytest.mark.parametrize("R,F,Tb,nb", [(3, 256, 32, 3), (3, 52, 48, 2)])
def test_each_optional_output_null_in_turn(gpu, pkg, R, F, Tb, nb):
    x, mask = _case("gamma", R, F, Tb, nb)
    want = _want("gamma", R, F, Tb, nb)
    blk = _block(pkg, "gamma", R, F, Tb, nb)
    for r in _both_routes(blk, _route_of(F)):
        for opt in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            got = _run(blk, x, opt=opt)
            assert [g is None for g in got[1:]] == [not o for o in opt] and _same(got, want), (r, opt)


def test_set_limits_and_set_mask_between_enqueued_calls(gpu, pkg):
    """two work_dev calls on one stream with set_limits / set_mask between them and no synchronisation: each call matches its own
    version; a refused update keeps the old values"""
    import torch
    R, F, Tb, nb = 3, 256, 32, 3
    x, mask1 = _case("gamma", R, F, Tb, nb)
    lim1 = _limits("gamma", Tb)
    lim2 = (8.0, 0.2, 3.0, 1.0, 1)
    mask2 = np.zeros(F, np.uint8)
    mask2[10:20] = 1
    w1 = _want("gamma", R, F, Tb, nb)
    w2 = ref.clean(x, Tb, *lim2, mask=mask2)
    assert not np.array_equal(w1[1], w2[1]) and not np.array_equal(w1[2], w2[2])
    d_x = torch.from_numpy(x.reshape(-1)).cuda()
    blk = _block(pkg, "gamma", R, F, Tb, nb)
    n = nb * Tb
    for r in _both_routes(blk, "slab"):
        blk.set_limits(*lim1)
        blk.set_mask(mask1)
        outs = [[torch.full((x.size,), float("nan"), device="cuda"), torch.full((nb * R * F,), -1, dtype=torch.int8, device="cuda"),
                 torch.full((n * R,), -1, dtype=torch.int8, device="cuda"), torch.full((2 * nb * R * F,), float("nan"), device="cuda")] for _ in range(2)]
        torch.cuda.synchronize()
        blk.work_device(n, [d_x], outs[0])
        blk.set_limits(*lim2)
        blk.set_mask(mask2)
        blk.work_device(n, [d_x], outs[1])
        torch.cuda.synchronize()
        for o, w in zip(outs, (w1, w2)):
            got = (o[0].cpu().numpy().reshape(n, R, F), o[1].cpu().numpy().view(np.uint8).reshape(nb, R, F),
                   o[2].cpu().numpy().view(np.uint8).reshape(n, R), o[3].cpu().numpy().reshape(nb, R, F, 2))
            assert _same(got, w), r
        assert blk.limits() == lim2 and np.array_equal(blk.mask(), mask2)
    for bad in ((0.0, 0.2, 3.0, 1.0, 1), (8.0, 3.0, 0.2, 1.0, 1), (8.0, 0.2, 3.0, -1.0, 1), (8.0, 0.2, 3.0, 1.0, 2), (8.0, float("nan"), 3.0, 1.0, 1)):
        with pytest.raises(pkg.Mi355Error):
            blk.set_limits(*bad)
    with pytest.raises(ValueError):
        blk.set_mask(mask2[:-1])
    assert pkg.lib().mi355_fbclean_set_mask(blk._h, None) == -1
    assert blk.limits() == lim2 and np.array_equal(blk.mask(), mask2)  # a refused update changes nothing
    assert _same(_run(blk, x), w2)


@pytest.mark.parametrize("R,F,Tb,nb", [(2, 512, 48, 2), (3, 52, 48, 2)])
def test_host_work_equals_the_reference(gpu, pkg, R, F, Tb, nb):
    x, mask = _case("gamma", R, F, Tb, nb)
    want = _want("gamma", R, F, Tb, nb)
    blk = _block(pkg, "gamma", R, F, Tb, nb)
    for r in _both_routes(blk, _route_of(F)):
        assert _same(blk.clean(x, flags=True), want), r
        assert _same((blk.clean(x),), want), r
        y = x.copy()  # in place on the host
        assert blk.work(nb * Tb, [y], [y]) == nb * Tb and _same((y,), want), r
    with pytest.raises(ValueError):
        blk.work(nb * Tb, [x.reshape(-1)[:-1]], [np.empty_like(x)])
    with pytest.raises(pkg.Mi355Error):
        blk.work(Tb + 1, [x], [np.empty_like(x)])


def test_host_work_in_pieces(gpu, pkg):
    """blocks of 1024 x 2 x 1024 floats = 8 MiB: work() sends the 3 blocks as 3 pieces"""
    R, F, Tb, nb = 2, 1024, 1024, 3
    x, mask = _case("gamma", R, F, Tb, nb)
    want = _want("gamma", R, F, Tb, nb)
    blk = _block(pkg, "gamma", R, F, Tb, nb)
    assert blk.route().startswith("slab ")
    assert _same(blk.clean(x, flags=True), want)


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    R, F, Tb = 2, 8, 16  # one block: 1024 bytes of samples, 16 cflags, 32 tflags, 128 bytes of stats
    blk = pkg.clFilterbankCleaner(*GPU_ARGS, R, F, Tb)
    L, h = pkg.lib(), blk._h
    buf = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    p = buf.data_ptr()
    vp = C.c_void_p
    W = L.mi355_fbclean_work_dev
    assert W(h, 16, vp(p + 2), vp(p + 4096), None, None, None, None) == -1             # in not 4-byte aligned
    assert W(h, 16, vp(p), vp(p + 4096 + 2), None, None, None, None) == -1             # out not 4-byte aligned
    assert W(h, 16, vp(p), vp(p + 4), None, None, None, None) == -1                    # out overlaps in without being in
    assert W(h, 16, vp(p + 1020), vp(p), None, None, None, None) == -1                 # in starts inside out
    assert W(h, 32, vp(p), vp(p + 2044), None, None, None, None) == -1                 # two blocks: 2048 bytes each
    assert W(h, 16, vp(p), vp(p + 4096), vp(p + 1023), None, None, None) == -1         # cflags inside in
    assert W(h, 16, vp(p), vp(p + 4096), vp(p + 8192), vp(p + 4096 + 1000), None, None) == -1   # tflags inside out
    assert W(h, 16, vp(p), vp(p + 4096), vp(p + 8192), vp(p + 8192 + 15), None, None) == -1     # tflags inside cflags
    assert W(h, 16, vp(p), vp(p + 4096), vp(p + 8192), vp(p + 9000), vp(p + 9024), None) == -1  # stats inside tflags
    assert W(h, 16, vp(p), vp(p + 4096), None, None, vp(p + 12288 + 4), None) == -1    # stats not 8-byte aligned
    assert W(h, 16, vp(p), vp(p), vp(p + 512), None, None, None) == -1                 # in place, but cflags inside the buffer
    assert W(h, 17, vp(p), vp(p + 4096), None, None, None, None) == -1                 # n is no multiple of Tb
    assert W(h, -16, vp(p), vp(p + 4096), None, None, None, None) == -1
    assert W(h, 16, None, vp(p + 4096), None, None, None, None) == -1
    assert W(h, 16, vp(p), None, None, None, None, None) == -1
    assert W(h, ((1 << 40) // 64 // 16 + 1) * 16, vp(p), vp(p), None, None, None, None) == -3  # samples of 64 bytes pass 2^40
    assert L.mi355_fbclean_work(h, 16, vp(p + 2), vp(p + 4096), None, None, None) == -1
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0  # nothing was launched


def test_zero_samples_is_a_no_op(gpu, pkg):
    import torch
    blk = pkg.clFilterbankCleaner(*GPU_ARGS, 2, 8, 16)
    out = torch.full((256,), 7.0, dtype=torch.float32, device="cuda")
    assert pkg.lib().mi355_fbclean_work_dev(blk._h, 0, None, C.c_void_p(out.data_ptr()), None, None, None, None) == 0
    assert pkg.lib().mi355_fbclean_work(blk._h, 0, None, None, None, None, None) == 0
    assert blk.work_device(0, [out], [out]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, whole blocks of items in and out, the optional flag streams"""
    mod = _pybind()
    R, F, Tb, nb = 2, 512, 48, 2
    n = nb * Tb
    x, mask = _case("gamma", R, F, Tb, nb)
    want = _want("gamma", R, F, Tb, nb)
    nd, lo, hi, td, z = _limits("gamma", Tb)
    fc = mod.clFilterbankCleaner(*GPU_ARGS, R, F, Tb, nd, lo, hi, td, bool(z), mask)
    assert fc.history() == 1 and fc.output_multiple() == Tb and fc.block_len() == Tb and fc.route().startswith("slab ")
    assert np.array_equal(fc.mask(), (mask != 0).astype(np.uint8)) and fc.limits() == [nd, lo, hi, td, float(z)]
    per_item = np.repeat(want[1], Tb, axis=0)  # output 2: the block's channel flags with every item
    for generic in (False, True):
        fc.set_generic(generic)
        assert fc.route().startswith("generic " if generic else "slab ")
        y = np.full_like(x, np.nan)
        tf = np.full((n, R), 0xFF, np.uint8)
        cf = np.full((n, R, F), 0xFF, np.uint8)
        assert fc.work(n, [x], [y, tf, cf]) == n
        assert _same((y, tf), (want[0], want[2])) and np.array_equal(cf, per_item)
        y[:] = np.nan
        assert fc.work(n, [x], [y]) == n and _same((y,), want)
    z2 = mod.clFilterbankCleaner(*GPU_ARGS, R, F, Tb)
    assert not z2.mask().any() and z2.limits() == [1.0, -INF, INF, INF, 0.0]
    z2.set_limits(nd, lo, hi, td, bool(z))
    z2.set_mask(mask)
    y = np.full_like(x, np.nan)
    assert z2.work(n, [x], [y]) == n and _same((y,), want)
    with pytest.raises(ValueError):
        z2.set_mask(mask[:-1])
    with pytest.raises(ValueError):
        z2.work(n, [x.reshape(-1)[:-1]], [y])  # one float fewer than the call reads
    with pytest.raises(ValueError):
        mod.clFilterbankCleaner(*GPU_ARGS, R, F, 40)


def test_cli_row(gpu):
    """test-clenabled-mi355 --fbclean-only prints the checksum of a small run on generated samples"""
    r = subprocess.run([CLI, "--fbclean-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    R, F, Tb, nb = 2, 256, 32, 3
    n = nb * Tb
    state, vals = 12345, np.empty(n * R * F, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    x = (vals + 1).astype(np.float32).reshape(n, R, F)
    mask = np.zeros(F, np.uint8)
    mask[7] = 1
    out, cf, tf, st = ref.clean(x, Tb, 1.0, 0.0, 1.0, 4.0, 1, mask)
    assert 0 < cf.mean() < 1 and cf[:, :, 7].all()
    u = np.uint64

    def wsum(a, m):
        a = a.reshape(-1).astype(u)
        return int(((np.arange(a.size, dtype=u) % u(m) + u(1)) * a).sum(dtype=u))

    want = (wsum(out.view(np.uint32), 7) + wsum(tf, 5) + wsum(cf, 3)) % (1 << 64)
    assert re.search(r"^clFilterbankCleaner checksum (\d+)$", r.stdout, re.M).group(1) == str(want), r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clFilterbankCleaner (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout


def _chain(pkg, sc, d_x, want_clean, want_peaks):
    """clFilterbankCleaner (in place) -> clDedisperser -> clPulseSearch on the device filterbank d_x, on both routes of the cleaner"""
    import torch
    R, F, D, K, Tb, H, n, n_dd, n_clean = (sc[k] for k in ("R", "F", "D", "K", "Tb", "H", "n", "n_dd", "n_clean"))
    S, nb = R * D, n // Tb
    fc = pkg.clFilterbankCleaner(*GPU_ARGS, R, F, Tb, sc["nd"], sc["sk_lo"], sc["sk_hi"], sc["td"], 1)
    dd = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, dedisp_ref.TIME_MAJOR, sc["tab"])
    ps = pkg.clPulseSearch(*GPU_ARGS, R, D, K, Tb, psearch_ref.TIME_MAJOR, None, sc["inv_sigma"])
    assert fc.floats_per_sample() == dd.in_floats_per_sample()
    got = None
    for r in _both_routes(fc, "slab"):
        wf, vf = guarded.guarded_output(n_clean * R * F, np.float32, guarded.pad_items(4, R * F), 0, "cuda")
        vf.copy_(d_x)
        wm, vm = guarded.guarded_output(S * n_dd, np.float32, guarded.pad_items(4, S), 0, "cuda")
        wo, vo = guarded.guarded_output(2 * nb * S, np.float32, guarded.pad_items(4, 2 * S), 0, "cuda")
        assert fc.work_device(n_clean, [vf], [vf]) == n_clean
        assert dd.work_device(n_dd, [vf], [vm]) == n_dd
        assert ps.work_device(nb, [vm], [vo]) == nb
        torch.cuda.synchronize()
        guarded.check_guards(wf, vf, "filterbank")
        guarded.check_guards(wm, vm, "series")
        guarded.check_guards(wo, vo, "peaks", interior=False)
        assert np.array_equal(guarded.to_numpy(vf).view(np.uint32), want_clean.reshape(-1).view(np.uint32)), r
        got = ps.peaks_of(vo).reshape(nb, S)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want_peaks).view(np.uint64)), r
    return got


def test_cleaner_feeds_the_search(gpu, pkg):
    """the end-to-end fixture of tests/test_fbclean.py on the device: clFilterbankCleaner -> clDedisperser -> clPulseSearch equal the three
    references chained bit for bit, and the strongest record is the injected pulse -- not the brighter zero-DM spike"""
    import torch
    sc = ref.search_scene()
    want_clean = ref.clean(sc["x"], sc["Tb"], sc["nd"], sc["sk_lo"], sc["sk_hi"], sc["td"], 1)[0]
    want = ref.search(sc, want_clean)
    got = _chain(pkg, sc, torch.from_numpy(sc["x"].reshape(-1)).cuda(), want_clean, want)
    b, s = np.unravel_index(np.argmax(got["snr"]), got.shape)
    assert (s, b, int(got["loc"][b, s])) == (sc["r0"] * sc["D"] + sc["d0"], sc["t0"] // sc["Tb"], (3 << 24) | (sc["t0"] % sc["Tb"]))


def test_beamformer_feeds_the_cleaner_and_the_search(gpu, pkg):
    """all four device blocks: int8 frames -> clBeamformer POWER (stokes_i) -> clFilterbankCleaner (in place on the beamformer's output) ->
    clDedisperser -> clPulseSearch, equal to beamform_ref, fbclean_ref, dedisp_ref and psearch_ref chained, bit for bit; nd = Ti npol"""
    import torch
    sc = dict(ref.search_scene())
    R, F, n_clean = sc["R"], sc["F"], sc["n_clean"]
    S, npol, Ti = 4, 2, 4
    rng = np.random.default_rng(99)
    frames = rng.integers(-8, 9, size=(n_clean * Ti, S, F, npol, 2), dtype=np.int8)
    w = np.zeros((F, npol, R, S, 2), np.int8)
    w[:, :, 0, :, 0] = 1
    w[:, :, 1] = rng.integers(-20, 21, size=(F, npol, S, 2), dtype=np.int8)
    power = beamform_ref.power(frames, w, Ti, True)  # [t][beam][chan] float32
    sc.update(nd=float(Ti * npol), sk_lo=0.7, sk_hi=1.3, td=3.0)  # flags 9 % of the cells of this uniform-voltage noise
    want_clean, cf, tf, st = ref.clean(power, sc["Tb"], sc["nd"], sc["sk_lo"], sc["sk_hi"], sc["td"], 1)
    assert 0 < cf.mean() < 0.5 and tf.any()
    want = ref.search(sc, want_clean)
    bf = pkg.clBeamformer(*GPU_ARGS, beamform_ref.POWER, npol, S, F, R, Ti, True, w)
    assert bf.out_items_per_unit() == R * F
    d_power = torch.full((n_clean * R * F,), float("nan"), dtype=torch.float32, device="cuda")
    assert bf.work_device(n_clean, [torch.from_numpy(frames.reshape(-1)).cuda()], [d_power]) == n_clean
    torch.cuda.synchronize()
    assert np.array_equal(d_power.cpu().numpy(), power.reshape(-1))
    _chain(pkg, sc, d_power, want_clean, want)
