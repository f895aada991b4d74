"""GPU: clPulseSearch against tests/psearch_ref.py (numpy float32, the contract's dyadic tree, S/N formula and 64-bit key order).  The
arithmetic is pinned, so every comparison of peaks is np.array_equal on the raw 8-byte records and candidate lists are compared as
sorted sets of raw 16-byte records; the one tolerance, for measure(), is derived in that test's docstring.  Every device call runs on
guard-banded buffers (tests/guarded.py), with NaN in the gaps of a pitched input, and the peaks buffer holds NaN bit patterns before the
call: a record the call never wrote would carry width index 0x7F.

Routes, as csrc/psearch.hip and the header state them:
  tiled    TRIAL_MAJOR K <= 12 (windows of 2048 samples for K <= 9, 4096 for K <= 11, 8192 for K = 12), TIME_MAJOR K <= 10 (32 series x
           1024 samples): k_ps_tiled; a tile delivers tt = window - (2^(K-1) - 1) outputs
  generic  every other K and every handle under set_generic(True): k_ps_gen
Every test asserts the route it expects through route().

Shapes stay small (at most 64 series, a few thousand samples; the one TRIAL_MAJOR K = 12 case that spans three tiles needs 14 347).

On an MI355X the file takes 3.5 s (61 tests)."""
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
import dedisp_ref
import guarded
import psearch_ref as ref

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")
FUSED_MAX = {ref.TRIAL_MAJOR: 12, ref.TIME_MAJOR: 10}


def _window(order, K):
    if order == ref.TIME_MAJOR:
        return 1024
    return 2048 if K <= 9 else 4096 if K <= 11 else 8192


def _route_of(order, K):
    return "tiled" if K <= FUSED_MAX[order] else "generic"


def _stats(S):
    """per-series statistics near the Gaussian fixture's (10, 3), different for every series"""
    s = np.arange(S, dtype=np.float32)
    return (np.float32(10) + np.float32(0.01) * s).astype(np.float32), (np.float32(1 / 3) * (1 + np.float32(0.001) * s)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(kind, S, T, Tb=16, seed=0):
    """x[S][T] float32, read-only"""
    rng = np.random.default_rng(9000 + seed + S * 3 + T * 5 + len(kind))
    x = (rng.standard_normal((S, T)) * 3 + 10).astype(np.float32)
    if kind == "integers":  # exact ties: the tie-break decides
        x = rng.integers(0, 4, (S, T)).astype(np.float32)
    elif kind == "nan":     # a single NaN
        x[S // 2, T // 3] = np.nan
    elif kind == "nanrun":  # a run that covers the whole of block 1 of the last series and that block's look-ahead
        x[S - 1, Tb - 3:] = np.nan
        x[0, 5] = np.nan
    elif kind == "inf":
        x[0, 7] = np.inf
        x[S - 1, T // 2] = np.inf
        x[S // 2, T - 1] = np.inf
    else:
        assert kind == "gaussian"
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _want(kind, S, K, Tb, nb, stats=True, seed=0):
    x = _case(kind, S, nb * Tb + ref.history(K), Tb, seed)
    m, g = _stats(S) if stats else (None, None)
    if kind == "integers":
        m = np.full(S, 1.5, np.float32)
    pk = ref.peaks(x, K, Tb, nb * Tb, m, g)
    pk.setflags(write=False)
    return pk


def _block(pkg, order, R, D, K, Tb, kind="gaussian", max_cands=0, stats=True):
    m, g = _stats(R * D) if stats else (None, None)
    if kind == "integers":
        m = np.full(R * D, 1.5, np.float32)
    return pkg.clPulseSearch(*GPU_ARGS, R, D, K, Tb, order, m, g, max_cands)


def _run(blk, x, nb, pitch=None, in_off=0, out_off=0, cand_off=0):
    """work_device on guard-banded buffers; x[S][>= nb Tb + Hs].  Returns (PEAK [nb][S], sorted candidate records, found, stored)"""
    import torch
    S, n = blk.num_series, nb * blk.block_len
    T = n + blk.history()
    buf = ref.to_order(np.asarray(x)[:, :T], blk.order, pitch)
    assert buf.size == blk.in_floats(nb, pitch)
    wi, vi = guarded.guarded_input(buf, guarded.pad_items(4, S), in_off, "cuda")
    wo, vo = guarded.guarded_output(2 * nb * S, np.float32, guarded.pad_items(4, 2 * S), out_off, "cuda")
    outs = [vo]
    if blk.max_cands:
        wc, vc = guarded.guarded_output(4 * blk.max_cands, np.float32, guarded.pad_items(4), cand_off, "cuda")
        wn, vn = guarded.guarded_output(2, np.float32, guarded.pad_items(4), cand_off, "cuda")
        outs += [vc, vn]
    assert blk.work_device(nb, [vi], outs, pitch) == nb
    torch.cuda.synchronize()
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "peaks", interior=False)
    pk = blk.peaks_of(vo).reshape(nb, S)
    assert (pk["loc"][(pk["loc"] >> 24) >= blk.num_widths] == 0xFFFFFFFF).all(), "an unwritten record"
    if not blk.max_cands:
        return pk, None, 0, 0
    guarded.check_guards(wc, vc, "candidates", interior=False)
    guarded.check_guards(wn, vn, "counts", interior=False)
    rec, found = blk.candidates()
    counts = guarded.to_numpy(vn).view(np.uint32)
    assert int(counts[0]) == found and int(counts[1]) == len(rec)
    # nothing behind the stored records was written
    assert (guarded.to_numpy(vc).view(np.uint32)[4 * len(rec):] == guarded.NAN_BITS).all()
    return pk, ref.sort_records(rec), found, len(rec)


def _both_routes(blk, expect_route):
    """yields the route names after asserting them: the geometry's own route, then the forced generic one"""
    assert blk.route().startswith(expect_route), blk.route()
    yield blk.route()
    blk.set_generic(True)
    assert blk.route().startswith("generic"), blk.route()
    yield blk.route()
    blk.set_generic(False)
    assert blk.route().startswith(expect_route)


def _same(a, b):
    """raw records, bit for bit"""
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_route_names_its_plan(gpu, pkg):
    blk = pkg.clPulseSearch(*GPU_ARGS, 64, 1024, 10, 1024, ref.TRIAL_MAJOR)
    assert blk.route() == "tiled trial R=64 D=1024 K=10 Tb=1024 ns=1 w=4096 tt=3585"
    assert (blk.num_series, blk.history()) == ref.plan(64, 1024, 10)[:2]
    blk = pkg.clPulseSearch(*GPU_ARGS, 64, 1024, 10, 1024, ref.TIME_MAJOR)
    assert blk.route() == "tiled time R=64 D=1024 K=10 Tb=1024 ns=32 w=1024 tt=513"
    blk.set_generic(True)
    assert blk.route() == "generic time R=64 D=1024 K=10 Tb=1024"
    assert pkg.clPulseSearch(*GPU_ARGS, 1, 3, 13, 16, ref.TRIAL_MAJOR).route() == "generic trial R=1 D=3 K=13 Tb=16"
    for order in FUSED_MAX:
        for K in range(1, 14):
            r = pkg.clPulseSearch(*GPU_ARGS, 1, 2, K, 16, order).route()
            assert r.startswith(_route_of(order, K)) and (r.startswith("generic") or " w=%d " % _window(order, K) in r), r


# order, R, D, K, Tb, nb.  tt = window - Hs outputs per tile: TIME_MAJOR 1024 - Hs; TRIAL_MAJOR 2048 / 4096 / 8192 - Hs
T_, X_ = ref.TRIAL_MAJOR, ref.TIME_MAJOR
FIXED = [
    (X_, 1, 1, 1, 16, 1),       # K = 1, S = 1, one block of the smallest length
    (X_, 1, 3, 2, 48, 5),       # K = 2, S = 3, Tb = 48
    (X_, 1, 33, 2, 16, 1),      # S = 33 crosses a group of 32 series
    (X_, 2, 17, 10, 16, 5),     # the largest fused K: Tb < Hs = 511; R = 2, D = 17
    (X_, 1, 33, 10, 1100, 1),   # a block over more than two tiles of 513
    (X_, 1, 3, 10, 250, 5),     # 1250 outputs: three tiles, blocks that straddle them (250 does not divide 513)
    (X_, 1, 3, 9, 300, 1),      # a tile of 769 that is not full
    (X_, 1, 1, 10, 48, 5),
    (X_, 1, 33, 11, 48, 5),     # one above: generic
    (X_, 2, 17, 11, 16, 1),
    (T_, 1, 1, 1, 16, 1),
    (T_, 1, 3, 2, 48, 5),
    (T_, 1, 33, 2, 16, 1),
    (T_, 2, 17, 12, 16, 5),     # the largest fused K (window 8192): Tb < Hs = 2047
    (T_, 1, 3, 12, 12300, 1),   # a block over more than two tiles of 6145
    (T_, 1, 33, 9, 700, 5),     # 3500 outputs: two tiles of 1793, blocks that straddle them
    (T_, 1, 1, 11, 5000, 1),    # the window of 4096: two tiles of 3073
    (T_, 1, 3, 10, 48, 5),
    (T_, 1, 33, 12, 16, 1),
    (T_, 1, 3, 13, 48, 5),      # one above: generic
    (T_, 2, 17, 13, 16, 1),
]


@pytest.mark.parametrize("order,R,D,K,Tb,nb", FIXED)
def test_fixed(gpu, pkg, order, R, D, K, Tb, nb):
    S = R * D
    x = _case("gaussian", S, nb * Tb + ref.history(K), Tb)
    want = _want("gaussian", S, K, Tb, nb)
    blk = _block(pkg, order, R, D, K, Tb)
    got = []
    for r in _both_routes(blk, _route_of(order, K)):
        got.append(_run(blk, x, nb)[0])
        assert _same(got[-1], want), (r, int(np.argmax(got[-1] != want)))
    assert _same(got[0], got[1])
    blk.stop()


@pytest.mark.parametrize("order", [X_, T_])
@pytest.mark.parametrize("kind", ["integers", "nan", "nanrun", "inf"])
@pytest.mark.parametrize("R,D,K,Tb,nb", [(2, 17, 5, 48, 5), (1, 3, 10, 300, 3)])
def test_data_sets(gpu, pkg, order, kind, R, D, K, Tb, nb):
    """exact ties, a single NaN, a NaN run over a whole block and +Inf samples: the reference's records on either route"""
    S = R * D
    x = _case(kind, S, nb * Tb + ref.history(K), Tb)
    want = _want(kind, S, K, Tb, nb)
    if kind == "nanrun":
        assert want["loc"][1, S - 1] == 0xFFFFFFFF and np.isneginf(want["snr"][1, S - 1]) and np.isfinite(want["snr"][:, 0]).all()
    if kind == "inf":
        assert np.isposinf(want["snr"]).sum() >= 3
    if kind == "integers":
        assert len(np.unique(want["snr"])) < want.size  # equal maxima in different blocks: the values tie all over
    blk = _block(pkg, order, R, D, K, Tb, kind)
    for r in _both_routes(blk, "tiled"):
        assert _same(_run(blk, x, nb)[0], want), r
    blk.stop()


@pytest.mark.parametrize("order,K", [(X_, 4), (X_, 10), (T_, 4), (T_, 12), (T_, 13), (X_, 11)])
def test_alignment_and_pitch(gpu, pkg, order, K):
    """`in` 4, 8 and 12 bytes past a 16-byte boundary, the outputs 8 bytes past one, and (TRIAL_MAJOR) in_pitch above n + Hs with NaN
    in the gaps: the bits of the aligned, dense call"""
    R, D, Tb, nb = 1, 3, 48, 2
    x = _case("gaussian", 3, nb * Tb + ref.history(K), Tb)
    want = _want("gaussian", 3, K, Tb, nb)
    T = nb * Tb + ref.history(K)
    blk = _block(pkg, order, R, D, K, Tb, max_cands=8)
    blk.set_threshold(np.sort(want["snr"].reshape(-1))[-3])
    cands = ref.candidates(want, np.sort(want["snr"].reshape(-1))[-3])
    for r in _both_routes(blk, _route_of(order, K)):
        for in_off, out_off, cand_off in ((0, 0, 0), (1, 0, 0), (2, 2, 0), (3, 0, 2), (1, 2, 2)):
            for pitch in ((None,) if order == X_ else (None, T + 1, T + 37)):
                pk, rec, found, stored = _run(blk, x, nb, pitch, in_off, out_off, cand_off)
                assert _same(pk, want) and np.array_equal(rec, cands) and found == stored == len(cands), (r, in_off, out_off, pitch)


@pytest.mark.parametrize("order,K", [(X_, 10), (T_, 12), (X_, 3), (T_, 13)])
def test_split_invariance(gpu, pkg, order, K):
    """5 blocks as one call, as five calls and as 2 + 3: identical peaks and an identical candidate set (block rebased by the caller)"""
    R, D, Tb, nb = 1, 3, 48, 5
    S, Hs = R * D, ref.history(K)
    x = _case("gaussian", S, nb * Tb + Hs, Tb)
    want = _want("gaussian", S, K, Tb, nb)
    thr = np.sort(want["snr"].reshape(-1))[-6]
    cands = ref.candidates(want, thr)
    blk = _block(pkg, order, R, D, K, Tb, max_cands=16)
    blk.set_threshold(thr)
    for r in _both_routes(blk, _route_of(order, K)):
        for split in ((5,), (1, 1, 1, 1, 1), (2, 3)):
            parts, recs, b0 = [], [], 0
            for m in split:
                pk, rec, found, stored = _run(blk, x[:, b0 * Tb:], m)
                rec = rec.copy()
                rec[:, 3] += b0
                parts.append(pk)
                recs.append(rec)
                b0 += m
            assert _same(np.concatenate(parts), want), (r, split)
            assert np.array_equal(ref.sort_records(np.concatenate(recs)), cands), (r, split)


def test_candidates_under_and_over_capacity(gpu, pkg):
    R, D, K, Tb, nb = 2, 17, 6, 48, 5
    S = R * D
    x = _case("gaussian", S, nb * Tb + ref.history(K), Tb)
    want = _want("gaussian", S, K, Tb, nb)
    thr = np.sort(want["snr"].reshape(-1))[-40]
    full = ref.candidates(want, thr)
    assert len(full) == 40
    full_set = {tuple(r) for r in full}
    for order in (X_, T_):
        for cap, expect_stored in ((64, 40), (40, 40), (7, 7)):
            blk = _block(pkg, order, R, D, K, Tb, max_cands=cap)
            assert _run(blk, x, nb)[2:] == (0, 0)  # the default threshold is +Inf: nothing is found
            blk.set_threshold(thr)
            for r in _both_routes(blk, "tiled"):
                pk, rec, found, stored = _run(blk, x, nb)
                assert _same(pk, want) and found == 40 and stored == expect_stored, (r, cap)  # counted in full, stored up to the capacity
                if cap >= 40:
                    assert np.array_equal(rec, full), (r, cap)
                else:  # a subset of the true set, no record twice
                    assert len({tuple(q) for q in rec}) == cap and {tuple(q) for q in rec} <= full_set, (r, cap)
            blk.set_threshold(-np.inf)  # every record is a candidate, the empty ones included
            assert _run(blk, x, nb)[2] == nb * S
            with pytest.raises(pkg.Mi355Error):
                blk.set_threshold(np.nan)
            blk.stop()


def test_set_stats_between_enqueued_calls(gpu, pkg):
    """two work_dev calls on one stream with set_stats between them and no synchronisation: each call matches its own version"""
    import torch
    R, D, K, Tb, nb = 2, 17, 6, 48, 5
    S = R * D
    x = _case("gaussian", S, nb * Tb + ref.history(K), Tb)
    m1, g1 = _stats(S)
    m2, g2 = (m1[::-1] * np.float32(0.5)).copy(), (g1 * np.float32(3)).astype(np.float32)
    w1, w2 = ref.peaks(x, K, Tb, nb * Tb, m1, g1), ref.peaks(x, K, Tb, nb * Tb, m2, g2)
    assert not _same(w1, w2)
    for order in (X_, T_):
        d_x = torch.from_numpy(ref.to_order(x, order)).cuda()
        blk = pkg.clPulseSearch(*GPU_ARGS, R, D, K, Tb, order, m1, g1)
        for r in _both_routes(blk, "tiled"):
            blk.set_stats(m1, g1)
            o1 = torch.full((nb * S,), -1, dtype=torch.int64, device="cuda")
            o2 = torch.full_like(o1, -1)
            torch.cuda.synchronize()
            blk.work_device(nb, [d_x], [o1])
            blk.set_stats(m2, g2)
            blk.work_device(nb, [d_x], [o2])
            torch.cuda.synchronize()
            assert _same(blk.peaks_of(o1).reshape(nb, S), w1) and _same(blk.peaks_of(o2).reshape(nb, S), w2), (r, order)
            assert np.array_equal(blk.stats()[0], m2) and np.array_equal(blk.stats()[1], g2)
        with pytest.raises(ValueError):
            blk.set_stats(m1[:-1], g1)
        assert np.array_equal(blk.stats()[0], m2)  # a refused update changes nothing


@pytest.mark.parametrize("order", [X_, T_])
def test_host_work_equals_device_work(gpu, pkg, order):
    R, D, K, Tb, nb = 2, 17, 6, 48, 5
    S = R * D
    x = _case("gaussian", S, nb * Tb + ref.history(K), Tb)
    want = _want("gaussian", S, K, Tb, nb)
    thr = np.sort(want["snr"].reshape(-1))[-9]
    blk = _block(pkg, order, R, D, K, Tb, max_cands=16)
    blk.set_threshold(thr)
    pitch = None if order == X_ else x.shape[1] + 5
    got = blk.search(ref.to_order(x, order, pitch), nb, pitch)
    rec, found = blk.candidates()
    dev = _run(blk, x, nb, pitch)
    assert _same(got.reshape(nb, S), want) and _same(dev[0], want)
    assert found == 9 and np.array_equal(ref.sort_records(rec), dev[1]) and np.array_equal(dev[1], ref.candidates(want, thr))
    with pytest.raises(ValueError):
        blk.search(ref.to_order(x, order, pitch)[:-1], nb, pitch)


@pytest.mark.parametrize("order", [X_, T_])
def test_host_work_in_pieces(gpu, pkg, order):
    """blocks of 64 x 10000 floats = 2.4 MiB: work() sends the 3 blocks as 3 pieces, each with its look-ahead; the candidates of the later
    pieces carry the block index of the call"""
    R, D, K, Tb, nb = 2, 32, 2, 10000, 3
    S = R * D
    x = _case("gaussian", S, nb * Tb + ref.history(K), Tb)
    want = _want("gaussian", S, K, Tb, nb)
    thr = np.sort(want["snr"].reshape(-1))[-20]
    cands = ref.candidates(want, thr)
    assert len(set(cands[:, 3])) == 3  # candidates in every piece
    blk = _block(pkg, order, R, D, K, Tb, max_cands=32)
    blk.set_threshold(thr)
    got = blk.search(ref.to_order(x, order), nb)
    rec, found = blk.candidates()
    assert _same(got.reshape(nb, S), want) and found == 20 and np.array_equal(ref.sort_records(rec), cands)
    small = _block(pkg, order, R, D, K, Tb, max_cands=5)  # over the capacity across pieces
    small.set_threshold(thr)
    small.search(ref.to_order(x, order), nb)
    rec, found = small.candidates()
    assert found == 20 and len(rec) == 5 and {tuple(q) for q in ref.sort_records(rec)} <= {tuple(q) for q in cands}


def test_refusals_launch_nothing(gpu, pkg):
    import torch
    R, D, K, Tb = 2, 4, 3, 16  # S = 8, Hs = 3: one block reads 19 x 8 floats = 608 bytes and writes 64 bytes
    tm = pkg.clPulseSearch(*GPU_ARGS, R, D, K, Tb, X_)
    tr = pkg.clPulseSearch(*GPU_ARGS, R, D, K, Tb, T_)
    L, h = pkg.lib(), tm._h
    buf = torch.zeros(1 << 16, dtype=torch.int8, device="cuda")
    p = buf.data_ptr()
    vp = C.c_void_p
    W = L.mi355_psearch_work_dev
    assert W(h, 16, vp(p + 2), 0, vp(p + 4096), None, 0, None, None) == -1            # in not 4-byte aligned
    assert W(h, 16, vp(p), 0, vp(p + 4096 + 4), None, 0, None, None) == -1            # peaks not 8-byte aligned
    assert W(h, 16, vp(p), 0, vp(p + 600), None, 0, None, None) == -1                 # peaks start inside the look-ahead
    assert W(h, 16, vp(p + 56), 0, vp(p), None, 0, None, None) == -1                  # in starts inside peaks
    assert W(h, 16, vp(p), 1, vp(p + 4096), None, 0, None, None) == -1                # TIME_MAJOR takes in_pitch 0 only
    assert W(tr._h, 16, vp(p), 18, vp(p + 4096), None, 0, None, None) == -1           # in_pitch < n + Hs
    assert W(tr._h, 16, vp(p), 100, vp(p + 2800), None, 0, None, None) == -1          # the pitched extent counts: 7 x 100 + 19 floats
    assert W(h, 17, vp(p), 0, vp(p + 4096), None, 0, None, None) == -1                # n is no multiple of Tb
    assert W(h, -16, vp(p), 0, vp(p + 4096), None, 0, None, None) == -1
    assert W(h, 16, None, 0, vp(p + 4096), None, 0, None, None) == -1
    assert W(h, 16, vp(p), 0, None, None, 0, None, None) == -1
    assert W(h, 16, vp(p), 0, vp(p + 4096), None, -1, None, None) == -1               # max_cands < 0
    assert W(h, 16, vp(p), 0, vp(p + 4096), vp(p + 8192), 4, None, None) == -1        # cands without counts
    assert W(h, 16, vp(p), 0, vp(p + 4096), vp(p + 8192 + 4), 4, vp(p + 9000), None) == -1   # cands not 8-byte aligned
    assert W(h, 16, vp(p), 0, vp(p + 4096), vp(p + 8192), 4, vp(p + 9004), None) == -1       # counts not 8-byte aligned
    assert W(h, 16, vp(p), 0, vp(p + 4096), vp(p + 4096 + 32), 4, vp(p + 9000), None) == -1  # cands inside peaks
    assert W(h, 16, vp(p), 0, vp(p + 4096), vp(p + 8192), 4, vp(p + 8192 + 56), None) == -1  # counts inside cands
    assert W(h, 16, vp(p), 0, vp(p + 4096), vp(p + 8192), 4, vp(p + 600), None) == -1        # counts inside in
    assert W(h, ((1 << 40) // 32 // 16 + 1) * 16, vp(p), 0, vp(p + 4096), None, 0, None, None) == -3  # n + Hs samples of 32 bytes pass 2^40
    assert W(tr._h, 16, vp(p), (1 << 40) // 32 + 1, vp(p + 4096), None, 0, None, None) == -3         # 8 series of that pitch pass 2^40
    assert L.mi355_psearch_work(h, 16, vp(p + 2), 0, vp(p + 4096), None, 0, None) == -1
    assert L.mi355_psearch_measure(h, 0, vp(p), 0, 1, vp(p), vp(p)) == -1
    torch.cuda.synchronize()
    assert int(buf.abs().max()) == 0  # nothing was launched


def test_zero_outputs_is_a_no_op(gpu, pkg):
    import torch
    blk = pkg.clPulseSearch(*GPU_ARGS, 2, 4, 3, 16)
    out = torch.full((256,), 7.0, dtype=torch.float32, device="cuda")
    assert pkg.lib().mi355_psearch_work_dev(blk._h, 0, None, 0, C.c_void_p(out.data_ptr()), None, 0, None, None) == 0
    assert pkg.lib().mi355_psearch_work(blk._h, 0, None, 0, None, None, 0, None) == 0
    assert blk.work_device(0, [out], [out]) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("order", [X_, T_])
def test_measure(gpu, pkg, order):
    """measure() against numpy float64 (tests/psearch_ref.py measure()).  The bound, for n samples of a series with A = sum |x|, u = 2^-53
    and g(m) = m u / (1 - m u) (the error constant of any float64 summation of m terms, Higham 4.4):
      mean:       both float64 means are within g(n) A / n of the true mean (a sum of n terms in some order, one division), so they differ
                  by at most 2 g(n) A / n; the device rounds its float64 mean once to float32: 2^-24 |mean|.
      inv_sigma:  sum (x - m')^2 = sum (x - m)^2 + n (m' - m)^2 exactly (the cross term vanishes at the true mean m), so a computed
                  variance is var (1 + e) with |e| <= g(n + 4) + (g(n) A / n)^2 / var (subtraction, square, n additions, division); 1 / sqrt
                  halves the relative error and adds two roundings.  Two such values differ by at most 2 (e / 2 + 2 u) relatively, and
                  the device rounds once to float32: 2^-24.
    With n = 3000 the float32 rounding is all but the whole of both bounds."""
    import torch
    R, D, n = 2, 17, 3000
    S = R * D
    x = _case("gaussian", S, n).copy()
    x[3] = np.float32(2.5)  # a constant series: variance 0 gives inv_sigma 0
    blk = pkg.clPulseSearch(*GPU_ARGS, R, D, 4, 16, order)
    m64, g64 = ref.measure(x, n)
    u = 2.0 ** -53
    A = np.abs(x.astype(np.float64)).sum(axis=1)
    gam = lambda m: m * u / (1 - m * u)
    dm = gam(n) * A / n
    var = ((x.astype(np.float64) - m64[:, None]) ** 2).mean(axis=1)
    bound_m = 2 * dm + 2.0 ** -24 * (np.abs(m64) + 2 * dm)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = gam(n + 4) + dm ** 2 / var
        bound_g = np.where(var == 0, 0.0, g64 * (2 * (e / 2 + 2 * u) * (1 + 1e-9) + 2.0 ** -24 * (1 + 1e-6)))
    pitch = None if order == X_ else n + 3
    buf = ref.to_order(x[:, :n], order, pitch)
    for src in (buf, torch.from_numpy(buf).cuda()):
        m, g = blk.measure(src, n, pitch)
        assert m.dtype == g.dtype == np.float32
        print("measure: mean error / bound %.3f, inv_sigma error / bound %.3f" % (
            np.max(np.abs(m - m64) / bound_m), np.max(np.abs(g - g64)[var > 0] / bound_g[var > 0])))
        assert (np.abs(m - m64) <= bound_m).all() and (np.abs(g - g64) <= bound_g).all()
        assert g[3] == 0 and m[3] == np.float32(2.5)
    # not installed: the statistics of the handle are still the defaults
    assert not blk.stats()[0].any() and (blk.stats()[1] == 1).all()
    blk.set_stats(m, g)
    assert np.array_equal(blk.stats()[0], m)


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pybind_block(gpu):
    """the C++ block as the scheduler calls it: work() on numpy buffers, n Tb + history() - 1 samples in, n items of R D records out"""
    mod = _pybind()
    R, D, K, Tb, nb = 2, 17, 6, 48, 5
    S = R * D
    x = _case("gaussian", S, nb * Tb + ref.history(K), Tb)
    want = _want("gaussian", S, K, Tb, nb)
    m, g = _stats(S)
    xin = ref.to_order(x, ref.TIME_MAJOR)
    ps = mod.clPulseSearch(*GPU_ARGS, R, D, K, Tb, m, g)
    assert ps.history() == ref.history(K) + 1 and ps.lookahead() == ref.history(K) and ps.decimation() == Tb and ps.route().startswith("tiled time")
    assert np.array_equal(ps.mean(), m) and np.array_equal(ps.inv_sigma(), g)
    y = np.zeros(nb * S, ref.PEAK)
    assert ps.work(nb, [xin], [y]) == nb and _same(y.reshape(nb, S), want)
    ps.set_generic(True)
    assert ps.route().startswith("generic")
    y[:] = 0
    assert ps.work(nb, [xin], [y]) == nb and _same(y.reshape(nb, S), want)
    z = mod.clPulseSearch(*GPU_ARGS, R, D, K, Tb)
    assert not z.mean().any() and (z.inv_sigma() == 1).all()
    z.set_stats(m, g)
    y[:] = 0
    assert z.work(nb, [xin], [y]) == nb and _same(y.reshape(nb, S), want)
    with pytest.raises(ValueError):
        z.set_stats(m[:-1], g)
    with pytest.raises(ValueError):
        z.work(nb, [xin[:-1]], [y])  # one float fewer than the call reads
    with pytest.raises(ValueError):
        mod.clPulseSearch(*GPU_ARGS, R, D, 14, Tb)


def test_cli_row(gpu):
    """test-clenabled-mi355 --psearch-only prints the checksum of a small run on generated samples"""
    r = subprocess.run([CLI, "--psearch-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    R, D, K, Tb, nb = 2, 5, 4, 32, 3
    T = nb * Tb + ref.history(K)
    state, vals = 12345, np.empty(T * R * D, np.int64)
    for i in range(vals.size):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        vals[i] = state >> 24
    x = (vals - 256 * (vals > 127)).astype(np.float32).reshape(T, R * D).T
    pk = ref.peaks(x, K, Tb, nb * Tb).reshape(-1)
    terms = (np.arange(pk.size, dtype=np.uint64) % np.uint64(7) + np.uint64(1)) * (pk["loc"].astype(np.uint64) + pk["snr"].view(np.uint32).astype(np.uint64))
    want = int(terms.sum(dtype=np.uint64))
    assert re.search(r"^clPulseSearch checksum (\d+)$", r.stdout, re.M).group(1) == str(want), r.stdout
    rows = [l for l in r.stdout.splitlines() if l.startswith("clPulseSearch (")]
    assert len(rows) == 2 and all(l.rstrip().endswith("ok") for l in rows), r.stdout


def test_dedisperser_feeds_the_pulse_search(gpu, pkg):
    """mi355_dedisp_delays -> clDedisperser -> clPulseSearch on the device, both orders: the peaks equal the two references chained bit
    for bit, and the global maximum is the injected (row, trial, width 8, time) -- which tests/test_psearch.py shows for the references
    alone"""
    import torch
    sc = ref.pulse_scene()
    R, F, D, K, Tb, nb, H, n, n_dd = (sc[k] for k in ("R", "F", "D", "K", "Tb", "nb", "H", "n", "n_dd"))
    S = R * D
    tab, top = pkg.dedisp_delays(1500.0, -300.0 / F, F, 1e-3, np.arange(D) * 4.0)
    assert np.array_equal(tab, sc["tab"]) and top == H
    y = dedisp_ref.dedisperse(sc["x"], tab, n_dd, dedisp_ref.TRIAL_MAJOR)
    want = ref.peaks(y.reshape(S, n_dd), K, Tb, n, None, sc["inv_sigma"])
    d_x = torch.from_numpy(sc["x"].reshape(-1)).cuda()
    for order in (X_, T_):
        dd = pkg.clDedisperser(*GPU_ARGS, R, F, D, H, order, tab)
        ps = pkg.clPulseSearch(*GPU_ARGS, R, D, K, Tb, order, None, sc["inv_sigma"])
        wm, vm = guarded.guarded_output(S * n_dd, np.float32, guarded.pad_items(4, S), 0, "cuda")
        wo, vo = guarded.guarded_output(2 * nb * S, np.float32, guarded.pad_items(4, 2 * S), 0, "cuda")
        for r in _both_routes(ps, "tiled"):
            assert dd.work_device(n_dd, [d_x], [vm]) == n_dd
            assert ps.work_device(nb, [vm], [vo]) == nb
            torch.cuda.synchronize()
            guarded.check_guards(wm, vm, "series")
            guarded.check_guards(wo, vo, "peaks", interior=False)
            got = ps.peaks_of(vo).reshape(nb, S)
            assert _same(got, want), (r, order)
            b, s = np.unravel_index(np.argmax(got["snr"]), got.shape)
            assert (s, b, int(got["loc"][b, s])) == (sc["r0"] * D + sc["d0"], sc["t0"] // Tb, (3 << 24) | (sc["t0"] % Tb))
