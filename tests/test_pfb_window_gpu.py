"""GPU: every kernel route of clPolyphaseChannelizer, step by step.  Per case and channel map (the identity, and one that repeats and omits
channels): the device path on guard-banded buffers (tests/guarded.py), last_route() names the kernel the case is about, every component of
every output is within the per-step bound of tests/pfb_ref.py, and a few planted non-finite items reach exactly the steps the contract of
include/mi355_clenabled.h allows: every mapped channel of the steps whose window [i R, i R + K) holds one, no step whose window stretched to
PMAXR rows of M items does not, every other step with the bits of the clean run.

Sizes come from the kernels' constants in csrc/pfb.hip and csrc/fft_mr.hip: the wave kernels (k_pfbs, k_pfbq, k_pfbw) work in groups of 16
steps, the staged kernel k_pfb in 4096 / M steps per workgroup iteration, k_pfb_fir in time ranges of max(8 taps-per-arm, ...) rounded up
to 8 steps (40 at 5 taps per arm, 160 at 20), k_pfb_branches_t in 8 steps per thread, k_pfb_branches in 256 outputs per workgroup, k_pfb_mr in
ranges of 8 steps for calls this short.  A call is a few of those and a ragged end, and long enough -- more than 2 PMAXR rows between the
planted items -- for the steps that must, may and must not be reached to be told apart.

Routes that a shape of the issue's grid does not take by itself:
  (64, 64, 32) and (256, 256, 5) run on k_pfbq (one workgroup per 16-step group) while a call has at most two groups per CU; the ring kernel
  k_pfbw takes the same shapes with MI355_PFB_SMALL=0 (read per call).  Both are run.
  (12, 3, 5) is 4-fold oversampled and runs on k_pfb_branches_t<8,4,4>; k_pfb_branches takes it with MI355_PFB_BRANCHES_PER_OUTPUT=1 (read per
  call), and (12, 4, 5), the nearest ratio the tiled kernel has no instance for, by itself.  Both are run.
"""
import functools

import numpy as np
import pytest

import guarded
import pfb_ref as ref
from conftest import GPU_ARGS

pytestmark = pytest.mark.gpu

RING = {"MI355_PFB_SMALL": "0"}
# (M, R, taps per arm, steps, environment, first kernel of last_route(), its tail for the identity map or None, steps per tile / range)
CASES = [
    (32, 32, 8, 229, {}, "k_pfbs<32,8>", "", 112),
    (64, 64, 32, 229, {}, "k_pfbq<64,32>", "", 112),
    (64, 64, 32, 229, RING, "k_pfbw<64,32>", "", 112),
    (256, 256, 5, 229, {}, "k_pfbq<256,8>", "", 112),
    (256, 256, 5, 229, RING, "k_pfbw<256,8>", "", 112),
    (512, 512, 8, 229, {}, "k_pfbw<512,8>", "", 112),
    (2, 2, 5, 2 * 2048 + 37, {}, "k_pfb<2,8>", "", 2048),
    (8, 8, 13, 2 * 512 + 37, {}, "k_pfb<8,16>", "", 512),
    (64, 32, 8, 460, {}, "k_pfbw<64,8,over=2>", "", 224),
    (128, 32, 16, 460, {}, "k_pfbw<128,16,over=4>", "", 192),
    (1024, 1024, 5, 229, {}, "k_pfb_fir<8>", " + clFFT", 120),
    (1024, 1024, 20, 333, {}, "k_pfb_fir<32>", " + clFFT", 160),
    (1024, 1024, 12, 229, {}, "k_pfb_branches_t<8,16,1>", " + clFFT", 112),
    (16, 8, 33, 458, {}, "k_pfb_branches_t<8,8,2>", " + clFFT", 224),
    (3, 2, 7, 300, {}, "k_pfb_branches", " + k_pfb_dft_map", 86),
    (12, 4, 5, 300, {}, "k_pfb_branches", " + k_pfb_dft_map", 128),
    (12, 3, 5, 400, {"MI355_PFB_BRANCHES_PER_OUTPUT": "1"}, "k_pfb_branches", " + k_pfb_dft_map", 192),
    (100, 100, 5, 413, {}, "k_pfb_mr<8>", "", 208),
    (48, 48, 9, 413, {}, "k_pfb_mr<16>", "", 208),
    (20, 20, 20, 413, {}, "k_pfb_mr<32>", "", 208),
    (360, 360, 5, 413, {}, "k_pfb_mr<8>", "", 208),
]


def _id(c):
    return "%d-%d-%d%s" % (c[0], c[1], c[2], "-ring" if c[4] is RING else "-per_output" if c[4] else "")


@functools.lru_cache(maxsize=None)
def _yard(M, R, P, steps):
    """taps, input, every channel of every step and the per-step bound: computed once per shape and shared (read-only)"""
    h = ref.make_taps(M, P)
    x = ref.make_input(h.size, R, steps)
    want, bnd = ref.channelize(h, M, R, list(range(M)), x, steps)
    want = want.reshape(steps, M)
    for a in (h, x, want, bnd):
        a.setflags(write=False)
    return h, x, want, bnd


def _run(blk, x, off, clean):
    import torch
    pad = guarded.pad_items(8)
    wi, vi = guarded.guarded_input(np.array(x), pad, off, device="cuda")  # (a copy: the shared yardstick arrays are read-only)
    wo, vo = guarded.guarded_output(blk.noutput(), np.complex64, pad, off, device="cuda")
    assert blk.work_device([vi], [vo]) == blk.noutput()
    torch.cuda.synchronize()
    route = blk.last_route()
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "output", interior=clean)  # (a planted item leaves non-finite outputs on purpose)
    return guarded.to_numpy(vo), route


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_values_and_reach_on_every_route(gpu, monkeypatch, case):
    M, R, P, steps, env, first, tail, tile = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert (steps * R) % M == 0
    h, x, want_all, bnd = _yard(M, R, P, steps)
    K = h.size
    rows = ref.pmaxr(-(-K // M))
    assert rows <= ref.PMAXR_CAP or P > 32
    pos, inf_at = ref.plant_positions(K, M, R, steps, tile)
    must, may = ref.reach(K, M, R, steps, pos), ref.reach(K, M, R, steps, pos, rows)
    assert 0 < must.sum() and may.sum() < steps and len(pos) >= 3, (pos, int(must.sum()), int(may.sum()))
    for which, cm in enumerate(ref.maps(M)):
        blk = gpu.clPolyphaseChannelizer(*GPU_ARGS, h, steps * R, M, R, cm)
        assert blk.last_route() == ""
        nmap = len(cm)
        clean, route = _run(blk, x, which, True)   # (the mapped run on buffers that are 8-byte aligned only)
        assert route.split(" + ")[0] == first, route
        if which == 0:
            assert route == first + tail, route
        want = want_all[:, cm].reshape(-1)
        r = ref.worst(clean, want, bnd, nmap)
        print("%-24s %-44s %4d mapped: worst error / bound %.3f over %d steps" % (_id(case), route, nmap, r, steps))
        assert ref.within(clean, want, bnd, nmap), r

        dirty, route2 = _run(blk, ref.plant(x, pos, inf_at), which, False)
        assert route2 == route
        d = dirty.reshape(steps, nmap)
        bad_re, bad_im = ~np.isfinite(d.real), ~np.isfinite(d.imag)
        bad_step = (bad_re | bad_im).any(axis=1)
        assert np.all(bad_re[must] & bad_im[must]), "finite outputs in steps whose window holds a planted item: steps %s" % (
            np.nonzero(must & ~(bad_re & bad_im).all(axis=1))[0][:8],)
        assert not np.any(bad_step & ~may), "non-finite outputs in steps %s, outside the %d rows planted items %s may reach" % (
            np.nonzero(bad_step & ~may)[0][:8], rows, pos)
        assert np.array_equal(d[~may].view(np.uint32), clean.reshape(steps, nmap)[~may].view(np.uint32))
        print("%-24s planted %s (+Inf at %d): %d steps must be non-finite, %d are, %d may be" % (_id(case), pos, pos[inf_at], must.sum(), bad_step.sum(), may.sum()))
        blk.stop()
