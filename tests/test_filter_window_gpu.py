"""GPU: every direct-form kernel of clFilter / clComplexFilter, output by output.  Per case: the device path on guard-banded buffers
(tests/guarded.py), last_route() names the kernel the case is about, every component of every output is within the per-output bound of
tests/fir_ref.py, and a few planted non-finite items reach exactly the outputs the contract of include/mi355_clenabled.h allows: all whose
window [m D, m D + K) holds one, none further than PAD items from one, every other output with the bits of the clean run.

Sizes come from the kernels' tile constants (csrc/filter.hip, restated in fir_ref.tile_items): two tiles and a ragged third, nothing larger.
How each kernel is reached (the launcher's choice is a rate model; the forcing switches used here are read per call):

  k_fir_td          fewer than 16 taps, or decimation 2 below 96 taps: its own choice (16 taps and more: tests/switch_cases.py, MI355_FIR_MFMA=0)
  k_fir_mfma<.,all> decimation 1 from 16 taps: its own choice
  k_fir_mfma<.,dec> decimations 2 ... 8 from 96 taps.  (200, 8, complex) does NOT take it by itself on a 16-byte aligned input -- the model puts
                    k_fir_dec2 ahead there -- so that shape runs with MI355_FIR_DEC_KERNEL=all, and (200, 3, complex), the nearest shape that
                    takes it by itself, runs beside it
  k_fir_dec2<.,even> its own choice at all three shapes
  k_fir_dec2<.,odd> MI355_FIR_DEC_KERNEL=lds
  k_fir_dec_lds     an input one item past a 16-byte boundary (8-byte aligned only), and again aligned with MI355_FIR_DEC2_OFF=1, both with
                    MI355_FIR_DEC_KERNEL=lds.  (65, 4) cannot reach it (decimations up to 8 of an input k_fir_dec2 does not take go to k_fir_td):
                    (65, 10), the nearest decimation that does, stands in for it.  (65, 3001): an odd decimation whose k_fir_dec2 tile would
                    hold one output -- tiles on odd samples, 16-byte loads at 8-byte alignment -- is routed here
  k_fir_td_dec      (33, 600) its own choice, (65, 40) MI355_FIR_DEC_KERNEL=per_output
"""
import functools

import numpy as np
import pytest

import fir_ref as ref
import guarded
from conftest import GPU_ARGS

pytestmark = pytest.mark.gpu

LDS = {"MI355_FIR_DEC_KERNEL": "lds"}
LDS_OFF2 = {"MI355_FIR_DEC_KERNEL": "lds", "MI355_FIR_DEC2_OFF": "1"}


def _cases():
    out = []
    for kern, shapes in ref.GRID.items():
        for K, D, c in shapes:
            if kern == "k_fir_td":
                out.append((kern, K, D, c, {}, 0))
            elif kern == "k_fir_mfma_all":
                out.append((kern, K, D, c, {}, 0))
            elif kern == "k_fir_mfma_dec":
                out.append((kern, K, D, c, {"MI355_FIR_DEC_KERNEL": "all"} if (K, D) == (200, 8) else {}, 0))
            elif kern == "k_fir_dec2_even":
                out.append((kern, K, D, c, {}, 0))
            elif kern == "k_fir_dec2_odd":
                out.append((kern, K, D, c, LDS, 0))
            elif kern == "k_fir_dec_lds":
                if D == 3001:
                    out.append((kern, K, D, c, LDS, 0))
                else:
                    out.append((kern, K, D, c, LDS, 1))
                    out.append((kern, K, D, c, LDS_OFF2, 0))
            else:
                out.append((kern, K, D, c, {"MI355_FIR_DEC_KERNEL": "per_output"} if (K, D) == (65, 40) else {}, 0))
    return out


def _id(c):
    return "%s-%d-%d%s%s%s" % (c[0], c[1], c[2], "-c" if c[3] else "", "-off1" if c[5] else "", "-dec2off" if "MI355_FIR_DEC2_OFF" in c[4] else "")


def _route(kern, K, D, c):
    """what last_route() must say"""
    ct = "complex" if c else "real"
    tile = ref.tile_items(kern, K, D) // D
    return {"k_fir_td": "k_fir_td<%s>" % ct, "k_fir_mfma_all": "k_fir_mfma<%s,all>" % ct, "k_fir_mfma_dec": "k_fir_mfma<%s,dec>" % ct,
            "k_fir_dec2_even": "k_fir_dec2<%s,even> tile_out=%d" % (ct, tile), "k_fir_dec2_odd": "k_fir_dec2<%s,odd> tile_out=%d" % (ct, tile),
            "k_fir_dec_lds": "k_fir_dec_lds<%s> tile_out=%d" % (ct, tile), "k_fir_td_dec": "k_fir_td_dec<%s>" % ct}[kern]


@functools.lru_cache(maxsize=None)
def _yard(kern, K, D, c):
    """the yardstick's result of a shape, computed once and shared (read-only)"""
    n = ref.nout(kern, K, D)
    h, x = ref.make_taps(K, c), ref.make_input(K, D, n)
    want, bnd = ref.fir(h, x, D, n), ref.bound(h, x, D, n)
    for a in (h, x, want, bnd):
        a.setflags(write=False)
    return n, h, x, want, bnd


def _run(blk, x, n, off, clean):
    import torch
    pad = guarded.pad_items(8)
    wi, vi = guarded.guarded_input(np.array(x), pad, off, device="cuda")  # (a copy: the shared yardstick arrays are read-only)
    wo, vo = guarded.guarded_output(n, np.complex64, pad, off, device="cuda")
    assert blk.work_device(n, [vi], [vo]) == n
    torch.cuda.synchronize()
    route = blk.last_route()
    guarded.check_guards(wi, vi, "input")
    guarded.check_guards(wo, vo, "output", interior=clean)  # (a planted item leaves non-finite outputs on purpose)
    return guarded.to_numpy(vo), route


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_values_and_reach_on_every_route(gpu, monkeypatch, case):
    kern, K, D, c, env, off = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, h, x, want, bnd = _yard(kern, K, D, c)
    blk = (gpu.clComplexFilter if c else gpu.clFilter)(*GPU_ARGS, D, h, 1, 0, True)
    assert blk.last_route() == ""
    clean, route = _run(blk, x, n, off, True)
    assert route == _route(kern, K, D, c)
    r = ref.worst(clean, want, bnd)
    print("%-34s %-40s worst error / bound %.3f over %d outputs" % (_id(case), route, r, n))
    assert ref.within(clean, want, bnd), r

    pos, inf_at = ref.plant_positions(K, D, n, ref.tile_items(kern, K, D))
    dirty, route2 = _run(blk, ref.plant(x, pos, inf_at), n, off, False)
    assert route2 == route
    must, may = ref.reach(K, D, n, pos), ref.reach(K, D, n, pos, ref.PAD)
    assert 0 < must.sum() and may.sum() < n, (pos, int(must.sum()), int(may.sum()))
    bad_re, bad_im = ~np.isfinite(dirty.real), ~np.isfinite(dirty.imag)
    bad = bad_re | bad_im
    assert not np.any(must & ~bad), "finite outputs whose window holds a planted item: %s" % np.nonzero(must & ~bad)[0][:8]
    assert not np.any(bad & ~may), "non-finite outputs further than PAD = %d items from every planted item %s: %s" % (
        ref.PAD, pos, np.nonzero(bad & ~may)[0][:8])
    assert np.all(bad_re[must] & bad_im[must])
    assert np.array_equal(dirty[~may].view(np.uint32), clean[~may].view(np.uint32))
    print("%-34s planted %s (+Inf at %d): %d outputs must be non-finite, %d are, %d may be" % (_id(case), pos, pos[inf_at], must.sum(), bad.sum(), may.sum()))
    blk.stop()


def test_fft_mode_reports_its_route(gpu):
    """The fast-convolution kernels are outside this file (an FFT spreads every sample over its block; their tolerance is the whole-call one):
    only that last_route() names them."""
    import torch
    h = ref.make_taps(65)
    blk = gpu.clFilter(*GPU_ARGS, 1, h, 1, 0, False)
    assert blk.last_route() == ""
    x = torch.from_numpy(ref.make_input(65, 1, 1000)).cuda()
    y = torch.full((1000,), float("nan"), dtype=torch.complex64, device="cuda")
    blk.work_device(1000, [x], [y])
    torch.cuda.synchronize()
    assert blk.last_route() == "k_ols<%d>" % blk.fftsize()
    assert ref.old_metric(y.cpu().numpy(), ref.fir(h, x.cpu().numpy(), 1, 1000)) <= 1e-5
    blk.stop()
