"""GPU: every kernel route of the X-engine's device path stays inside the caller's buffers (the X-engine half of
tests/test_device_bounds_gpu.py; the two files together are the inventory of DESIGN.md, 'Buffer contract').

Every case puts the input and the output into guarded allocations (tests/guarded.py): the integer sentinel around int8 and packed 4-bit
input (bytes 5B 5A 5A 5A: a stray sample that enters a sum changes it), NaN around complex-float input, the sentinel around the
output, NaN inside it (or a prior matrix for the accumulate form).  Pads: max(64 KiB, one time step of the input / one channel's matrix
of the output), at most 1 MiB.  After the call: the pads bit for bit, the interior against the oracle (int8 bit for bit against the exact
integer sums, complex float and packed 4-bit to 1e-5), and last_route() against the route the case is named for -- a case that falls
through to another kernel fails.  Outputs run 0 and 1 item past a 16-byte boundary; inputs at offset 0, and in a group of their own at
4 / 8 / 12 bytes (int8) and 8 bytes (complex float), where the launcher takes the generic kernels.

ROUTES is the table of every label mi355_xe_route_set records, with the kernels behind it; test_every_route_label_is_accounted_for
(CPU) reads the labels out of csrc/xengine*.hip and fails when one is missing here or asserted by no case.  Two labels serve two corner
turns each: 'k_xe_turn+k_xe_corr_lds' and 'k_xe_turn+k_xe_corr' are recorded for k_xe_turn_lds (rows of whole 128-byte lines AND a
16-byte aligned input, launch_xe_body's fast_turn) and for k_xe_turn (anything else); the ids say which one the geometry and the input
offset select.  k_xe_pad_rows / k_xe_pad_rows8 run in front of whatever kernel follows (odd channel counts, complex rows that are
copied): the ids name them too.

Not visible to guard bands: a load past the input whose value is discarded (early touches, prefetch).  The library's own workspaces
(tiles, partial sums, padded rows, the shard's receive buffers) are not the caller's and cannot be guarded from here.
"""
import glob
import os
import re

import numpy as np
import pytest
import torch

from conftest import GPU_ARGS, crandn, relerr
from guarded import check_guards, guarded_input, guarded_output, pad_items, prefill_output, to_numpy
from test_device_bounds_gpu import _host_check, _host_out, _run_offsets, _setenv

gpu_test = pytest.mark.gpu
TOL = 1e-5   # complex float and packed 4-bit: the bound of tests/test_xengine_gpu.py
DEV = "cuda"
OUT2 = ((0, 0), (0, 1))  # (input offset, output offset) in items: the output 16-byte aligned and 8-byte aligned only

# label -> the kernels it stands for
ROUTES = {
    "k_xe_i8_fused": "k_xe_i8_fused, one launch; with time ranges the in-launch reduction (route field in_launch_reduce = 1)",
    "k_xe_i8_fused+k_xe_i8_reduce": "k_xe_i8_fused over time ranges, then k_xe_i8_reduce",
    "k_xe_i8_lines": "k_xe_i8_lines<false>",
    "k_xe_i8_lines<split>": "k_xe_i8_lines<true>: time ranges combined in the launch",
    "k_xe_i8_lines<2 pol>": "k_xe_i8_lines<false, 2>",
    "k_xe_turn_lds+k_xe_corr_sb": "k_xe_turn_lds, then k_xe_corr_sb (65 .. 256 rows)",
    "k_xe_turn+k_xe_corr_sb": "k_xe_turn, then k_xe_corr_sb",
    "k_xe_turn+k_xe_corr_lds": "k_xe_turn_lds OR k_xe_turn (see the module docstring), then k_xe_corr_lds",
    "k_xe_turn+k_xe_corr": "k_xe_turn_lds OR k_xe_turn, then k_xe_corr",
    "k_xe_f32_fused+k_xe_reduce": "k_xe_f32_fused, then k_xe_reduce",
    "k_xe_turn_f32+k_xe_corr_f32": "k_xe_turn_f32, then k_xe_corr_f32",
    "k_xe_cf32": "k_xe_cf32 (vector ALU)",
}
ASSERTED = set()  # labels some case of this file asserts (filled while the tables below are built)


def _param(table, tag, label, *rest):
    assert label in ROUTES, label
    ASSERTED.add(label)
    table.append(pytest.param(label, *rest, id="%s-%s" % (tag, label.replace("+", "_then_"))))


def _block(gpu, kind, N, F, T, npol):
    dt = {"i8": gpu.DTYPE_BYTE, "cf32": gpu.DTYPE_COMPLEX, "p4": gpu.DTYPE_PACKEDXY}[kind]
    return gpu.clXEngine(*GPU_ARGS, False, dt, npol, N, gpu.CLXCORR_TRIANGULAR_ORDER, 0, F, T, [])


def _nb(N, npol):
    """items of one channel's matrix"""
    return N * (N + 1) // 2 * npol * npol


_DATA = {}


def _data(oracle, kind, N, F, T, npol, nint=1):
    """(windows of input [nint, items], [(window, first channel, last channel, oracle result)]); computed once per geometry and left
    unchanged.  One window: the whole matrix.  Several: every window while the oracle's work stays below ~ 1e8 products, else the first,
    the middle and the last window, and of those the first, the middle and the last 64 channels where one window alone is above 3e7
    (channels are independent: the oracle runs on a 64-channel slice of the input)."""
    key = (kind, N, F, T, npol, nint)
    if key not in _DATA:
        if len(_DATA) >= 6:
            _DATA.pop(next(iter(_DATA)))
        rng = np.random.default_rng(N * 1000 + F * 7 + T + npol + nint)
        rows = N * npol
        cost = rows * (rows + 1) // 2 * F * T
        wins = range(nint) if cost * nint <= 1e8 else sorted({0, nint // 2, nint - 1})
        if kind == "cf32":
            x = crandn(rng, nint * T * N * F * npol).reshape(nint, -1)
            refs = [(i, 0, F, oracle.xengine_cf32(N, F, npol, T, x[i])) for i in wins]
        elif kind == "p4":
            x = rng.integers(0, 256, size=(nint, T * N * F * 2), dtype=np.int64).astype(np.uint8)
            refs = [(i, 0, F, oracle.xengine_packed4(N, F, T, x[i])) for i in wins]
        else:
            x = rng.integers(-128, 128, size=(nint, T, N, F, npol * 2), dtype=np.int64).astype(np.int8)
            mid = (F // 2) // 64 * 64
            spans = sorted({(0, 64), (mid, mid + 64), (F - 64, F)}) if nint > 1 and cost > 3e7 and F > 192 else [(0, F)]
            refs = [(i, f0, f1, oracle.xengine_ichar(N, f1 - f0, npol, T, np.ascontiguousarray(x[i, :, :, f0:f1]).reshape(-1), exact=True))
                    for i in wins for f0, f1 in spans]
            x = x.reshape(nint, -1)
        _DATA[key] = (x, refs)
    return _DATA[key]


def _prior(kind, N, F, npol, seed=0):
    """what the accumulate form adds into: a matrix of the size of the results (int8 sums of T frames scaled by 1 / 127^2 are of order
    sqrt(T); complex-float sums likewise)"""
    rng = np.random.default_rng(seed + N + F)
    return (crandn(rng, F * _nb(N, npol)) * np.float32(8.0)).astype(np.complex64)


def _with_prior(oracle, kind, N, F, T, npol, x, prior):
    acc = prior.copy()
    if kind == "cf32":
        return oracle.xengine_cf32(N, F, npol, T, x, acc=acc)
    if kind == "p4":
        return oracle.xengine_packed4(N, F, T, x, acc=acc)
    return oracle.xengine_ichar(N, F, npol, T, x, exact=True, acc=acc)


def _route(blk, label, want):
    r = blk.last_route()
    print("route:", r)
    assert r["kernel"] == label, r
    for k, v in want.items():  # a field's value, or under "all" a condition over the whole record
        assert (v(r) if k == "all" else r[k] == v), (k, r)
    return r


def _grouped(x, T, N, F, npol, ng):
    """[t][station] -> [group][t][station in group] (one window)"""
    return np.ascontiguousarray(x.reshape(T, N // ng, ng, F, npol * 2).transpose(1, 0, 2, 3, 4)).reshape(-1)


def _one_window(gpu, oracle, kind, label, geo, want, acc=False, spg=None, offsets=OUT2, labels=None):
    """one window through xcorrelate_device at every (input, output) offset; labels: the route per offset pair where it differs.  int8: the
    first run bit for bit against the oracle, every later run bit for bit against the first (_run_offsets, bitwise)"""
    N, F, T, npol = geo
    x, refs = _data(oracle, kind, N, F, T, npol)
    x0, ref = x[0], refs[0][3]
    prior = _prior(kind, N, F, npol) if acc else None
    if acc:
        ref = _with_prior(oracle, kind, N, F, T, npol, x0, prior)
    blk = _block(gpu, kind, N, F, T, npol)
    per = blk.get_output_buffer_size()
    assert per == F * _nb(N, npol) and blk.input_bytes() == x0.nbytes
    xin = _grouped(x0, T, N, F, npol, spg) if spg else x0
    payload = xin.view(np.int8) if kind == "p4" else xin
    step = x0.size // T  # items of one time step
    seen = []

    def call(i, o):
        if acc:
            prefill_output(o[0], prior)
        blk.xcorrelate_device(i[0], o[0], accumulate=acc, stations_per_group=spg)
        seen.append(_route(blk, labels[len(seen)] if labels else label, want))

    def check(outs):
        if kind == "i8":
            bad = np.flatnonzero(outs[0].view(np.uint32) != ref.view(np.uint32))
            assert bad.size == 0, "first differing float %d of %d" % (bad[0], 2 * per)
        else:
            err = relerr(outs[0], ref)
            print("relerr %s %s %.3g" % (label, geo, err))
            assert err <= TOL

    _run_offsets(call, [(payload, step)], [(per, np.complex64, _nb(N, npol))], offsets, check, bitwise=(kind == "i8"))
    assert len(seen) == len(offsets)
    blk.stop()


# ------------------------------------------------------------------------------------------------------------ int8, one window

I8 = []


def _i8(tag, label, geo, env=None, want=None, acc=False, spg=None):
    sw = "".join("-%s=%s" % (k.replace("MI355_XE_", ""), v) for k, v in (env or {}).items())
    _param(I8, "%s%s-%dx%dx%dx%d%s%s" % (tag, sw, *geo, "-accumulate" if acc else "", "-groups_of_%d" % spg if spg else ""),
           label, geo, env or {}, want or {}, acc, spg)


_ONE = {"tsplit": 1, "windows": 1, "launches": 1}
for _tag, _geo in (("one_row_tile", (5, 64, 32, 1)), ("two_row_tiles_ragged_time", (20, 64, 33, 1)),
                   ("four_row_tiles_from_three_80_byte_rows", (33, 40, 100, 1)), ("two_pol_ragged_time", (16, 20, 31, 2)),
                   ("four_row_tiles", (64, 64, 64, 1)), ("rows_of_one_16_byte_piece", (64, 8, 40, 1))):
    _i8("fused_direct-" + _tag, "k_xe_i8_fused", _geo, want=_ONE)
_i8("fused_direct", "k_xe_i8_fused", (64, 64, 64, 1), want=_ONE, acc=True)
for _geo in ((64, 64, 256, 1), (32, 64, 512, 2)):
    for _acc in ((False, True) if _geo[3] == 1 else (False,)):
        _i8("fused_time_ranges", "k_xe_i8_fused+k_xe_i8_reduce", _geo, {"MI355_XE_TSPLIT": "4", "MI355_XE_INKERNEL_REDUCE": "0"},
            {"tsplit": 4, "in_launch_reduce": 0}, acc=_acc)
        _i8("fused_time_ranges_in_launch_reduction", "k_xe_i8_fused", _geo, {"MI355_XE_TSPLIT": "4", "MI355_XE_INKERNEL_REDUCE": "1"},
            {"tsplit": 4, "in_launch_reduce": 1}, acc=_acc)
_LN = {"MI355_XE_LINES_MIN_UNITS": "4"}
_i8("whole_line", "k_xe_i8_lines", (64, 64, 32, 1), _LN, _ONE)
_i8("whole_line", "k_xe_i8_lines", (64, 128, 96, 1), _LN, _ONE)
_i8("whole_line", "k_xe_i8_lines<2 pol>", (64, 32, 32, 2), _LN, _ONE)
_i8("whole_line", "k_xe_i8_lines<split>", (64, 128, 128, 1), {"MI355_XE_LINES_SPLIT_ANY": "1", "MI355_XE_TSPLIT": "2"}, {"tsplit": 2, "in_launch_reduce": 1})
# at most 64 rows through the two kernels.  k_xe_turn_lds: 128-byte rows, aligned input.  k_xe_turn: rows of 8 bytes
_NF = {"MI355_XE_NO_FUSED": "1"}
for _acc in (False, True):
    _i8("k_xe_turn_lds_by_128_byte_rows", "k_xe_turn+k_xe_corr_lds", (64, 64, 64, 1), _NF, acc=_acc)
    _i8("k_xe_turn_lds_by_128_byte_rows", "k_xe_turn+k_xe_corr", (64, 64, 64, 1), dict(_NF, MI355_XE_NO_LDS="1"), acc=_acc)
_i8("k_xe_turn_by_8_byte_rows", "k_xe_turn+k_xe_corr_lds", (17, 4, 65, 1))
# (33 x 2 polarisations are 66 rows: five row tiles, six after the padding at create, so the correlation is k_xe_corr_sb's, not k_xe_corr_lds';
#  the 40-byte rows keep the slow corner turn; 32 x 2 = 64 rows below is the two-polarisation shape that stays with k_xe_corr_lds)
_i8("k_xe_turn_by_40_byte_rows-six_row_tiles_from_five", "k_xe_turn+k_xe_corr_sb", (33, 10, 130, 2))
_i8("k_xe_turn_by_40_byte_rows", "k_xe_turn+k_xe_corr_lds", (32, 10, 130, 2))
# odd channel counts: k_xe_pad_rows first.  7 channels become 8 = one 16-byte piece, which the fused kernel then reads from the padded copy;
# 5 channels become 6 (12-byte rows) and 1 becomes 2: the two kernels
_i8("k_xe_pad_rows", "k_xe_i8_fused", (9, 7, 50, 1), want=_ONE)
_i8("k_xe_pad_rows", "k_xe_i8_fused", (12, 7, 70, 1), want=_ONE)
_i8("k_xe_pad_rows-k_xe_turn", "k_xe_turn+k_xe_corr", (3, 1, 2, 1))
_i8("k_xe_pad_rows-k_xe_turn", "k_xe_turn+k_xe_corr", (9, 5, 50, 1))
# more than 64 rows
_SB, _SBS = "k_xe_turn_lds+k_xe_corr_sb", "k_xe_turn+k_xe_corr_sb"
for _tag, _lab, _geo, _w in (("8_row_tiles", _SB, (128, 64, 32, 1), {}), ("10_row_tiles_from_9", _SB, (130, 64, 32, 1), {}),
                             ("12_row_tiles_from_11_two_pol_ragged_time", _SB, (81, 32, 33, 2), {}), ("14_row_tiles_from_13", _SB, (200, 64, 32, 1), {}),
                             ("16_row_tiles-k_xe_turn_by_32_byte_rows", _SBS, (256, 16, 32, 1), {}),
                             ("10_row_tiles-k_xe_turn_by_20_byte_rows", _SBS, (160, 10, 40, 1), {}),
                             ("10_row_tiles_from_9-k_xe_pad_rows-k_xe_turn", _SBS, (129, 3, 65, 1), {}),
                             ("several_channels_per_workgroup", _SB, (130, 320, 32, 1), {"all": lambda r: r["units_per_workgroup"] > 1})):
    _i8("above_64_rows-" + _tag, _lab, _geo, want=_w)
_i8("above_64_rows", _SB, (128, 64, 32, 1), acc=True)
_i8("above_64_rows-k_xe_turn_lds", "k_xe_turn+k_xe_corr_lds", (128, 64, 32, 1), {"MI355_XE_NO_SB": "1"})
_i8("above_64_rows-k_xe_turn_lds", "k_xe_turn+k_xe_corr_lds", (128, 64, 32, 1), {"MI355_XE_NO_SB8": "1"})
_i8("above_64_rows", _SBS, (128, 64, 32, 1), {"MI355_XE_SLOW_TURN": "1"})
_i8("above_64_rows-three_channel_slabs", _SB, (128, 192, 32, 1), {"MI355_XE_SLABS": "3"}, {"launches": 3})
_i8("group_major", "k_xe_i8_fused", (64, 64, 64, 1), want=_ONE, spg=16)


@gpu_test
@pytest.mark.parametrize("label,geo,env,want,acc,spg", I8)
def test_int8_window_stays_inside_its_buffers(gpu, oracle, monkeypatch, label, geo, env, want, acc, spg):
    _setenv(monkeypatch, env)
    _one_window(gpu, oracle, "i8", label, geo, want, acc, spg)


# (geometry, route of the aligned run, route of the runs at 4 / 8 / 12 bytes): the fused and whole-line kernels, k_xe_turn_lds and the
# matrix-core complex-float kernels want 16 bytes; anything else goes to k_xe_turn (int8) and k_xe_cf32 (complex float)
UNALIGNED = []
_param(UNALIGNED, "int8-64x64x64x1-k_xe_turn_by_input_offset", "k_xe_turn+k_xe_corr_lds", "i8", (64, 64, 64, 1), "k_xe_i8_fused", (4, 8, 12))
_param(UNALIGNED, "int8-20x64x33x1-k_xe_turn_by_input_offset", "k_xe_turn+k_xe_corr_lds", "i8", (20, 64, 33, 1), "k_xe_i8_fused", (4, 8, 12))
_param(UNALIGNED, "int8-128x64x32x1-k_xe_turn_by_input_offset", "k_xe_turn+k_xe_corr_sb", "i8", (128, 64, 32, 1), "k_xe_turn_lds+k_xe_corr_sb", (4, 8, 12))
_param(UNALIGNED, "int8-9x5x50x1-k_xe_pad_rows", "k_xe_turn+k_xe_corr", "i8", (9, 5, 50, 1), "k_xe_turn+k_xe_corr", (4, 8, 12))
_param(UNALIGNED, "complex_float-16x16x64x1", "k_xe_cf32", "cf32", (16, 16, 64, 1), "k_xe_f32_fused+k_xe_reduce", (1,))
_param(UNALIGNED, "complex_float-70x16x20x2", "k_xe_cf32", "cf32", (70, 16, 20, 2), "k_xe_turn_f32+k_xe_corr_f32", (1,))


@gpu_test
@pytest.mark.parametrize("label,kind,geo,aligned_label,in_offs", UNALIGNED)
def test_unaligned_input_takes_the_generic_kernels_and_stays_inside(gpu, oracle, label, kind, geo, aligned_label, in_offs):
    """input offsets in items past a 16-byte boundary (int8: bytes; complex float: 8 bytes), the output alternating between 16- and 8-byte
    alignment.  The first run is the aligned one, on the route the geometry has by itself: it is compared with the oracle, and every int8
    run at an offset must equal it bit for bit (complex float: each run against the oracle)."""
    offsets = [(0, 0)] + [(o, k & 1) for k, o in enumerate(in_offs, 1)]
    _one_window(gpu, oracle, kind, label, geo, {}, offsets=offsets, labels=[aligned_label] + [label] * len(in_offs))


# ------------------------------------------------------------------------------------------------------------- packed 4-bit

P4 = []
_param(P4, "5x6x70-k_xe_turn_by_12_byte_rows", "k_xe_turn+k_xe_corr", (5, 6, 70))
_param(P4, "6x5x40-k_xe_pad_rows-k_xe_turn", "k_xe_turn+k_xe_corr", (6, 5, 40))
_param(P4, "80x64x32-160_rows-k_xe_turn_lds", "k_xe_turn_lds+k_xe_corr_sb", (80, 64, 32))


@gpu_test
@pytest.mark.parametrize("label,geo", P4)
def test_packed4_window_stays_inside_its_buffers(gpu, oracle, label, geo):
    N, F, T = geo
    _one_window(gpu, oracle, "p4", label, (N, F, T, 2), {})


# ------------------------------------------------------------------------------------------------------------ complex float

CF = []


def _cf(tag, label, geo, env=None, want=None, acc=False):
    sw = "".join("-%s=%s" % (k.replace("MI355_XE_CF32_", ""), v) for k, v in (env or {}).items())
    _param(CF, "%s%s-%dx%dx%dx%d%s" % (tag, sw, *geo, "-accumulate" if acc else ""), label, geo, env or {}, want or {}, acc)


_FU, _TK, _VA = "k_xe_f32_fused+k_xe_reduce", "k_xe_turn_f32+k_xe_corr_f32", "k_xe_cf32"
# (8 channels x one polarisation are 64-byte rows and 24 channels 192-byte rows: padded to whole lines at create and read as given,
#  like the ragged rows below)
for _geo in ((5, 8, 3, 1), (8, 8, 20, 2), (24, 16, 130, 2), (64, 24, 100, 1)):
    _cf("fused", _FU, _geo)
_cf("fused", _FU, (16, 16, 64, 1), {"MI355_XE_CF32_CH": "4"})
_cf("fused", _FU, (16, 16, 64, 1), {"MI355_XE_CF32_TSPLIT": "1"}, {"tsplit": 1})
_cf("fused", _FU, (16, 16, 64, 1), acc=True)
for _geo in ((20, 10, 64, 1), (12, 50, 40, 2)):
    _cf("ragged_rows_read_in_place", _FU, _geo)
    _cf("ragged_rows-k_xe_pad_rows8", _FU, _geo, {"MI355_XE_CF32_PAD_COPY": "1"})
    _cf("ragged_rows_unpadded", _VA, _geo, {"MI355_XE_CF32_NO_PAD": "1"})
_cf("two_kernels", _TK, (16, 16, 64, 2), {"MI355_XE_CF32_TWO_KERNELS": "1"})
_cf("two_kernels", _TK, (16, 16, 64, 2), {"MI355_XE_CF32_TWO_KERNELS": "1"}, acc=True)
_cf("two_kernels-140_rows", _TK, (70, 16, 20, 2))
_cf("two_kernels-several_workgroups_per_channel", _TK, (130, 16, 48, 1))
_cf("vector_alu-k_xe_pad_rows8-260_rows", _VA, (260, 10, 24, 1))
_cf("vector_alu", _VA, (20, 37, 64, 1), {"MI355_XE_CF32_VALU": "1"})
_cf("vector_alu", _VA, (20, 37, 64, 1), {"MI355_XE_CF32_VALU": "1"}, acc=True)


@gpu_test
@pytest.mark.parametrize("label,geo,env,want,acc", CF)
def test_complex_float_window_stays_inside_its_buffers(gpu, oracle, monkeypatch, label, geo, env, want, acc):
    _setenv(monkeypatch, env)  # (MI355_XE_CF32_NO_PAD is read at create: the block is created below)
    _one_window(gpu, oracle, "cf32", label, geo, want, acc)


# ----------------------------------------------------------------------------------------------- several windows in one call

WIN = []


def _win(tag, label, kind, geo, nint, env=None, want=None, spg=None):
    sw = "".join("-%s=%s" % (k.replace("MI355_XE_", ""), v) for k, v in (env or {}).items())
    _param(WIN, "%s%s-%dx%dx%dx%d-%d_windows%s" % (tag, sw, *geo, nint, "-groups_of_%d" % spg if spg else ""), label, kind, geo, nint,
           env or {}, want or {}, spg)


_NL = {"MI355_XE_NO_LINES": "1"}
_win("fused_batched", "k_xe_i8_fused", "i8", (64, 64, 32, 1), 3, _NL, {"windows": 3, "launches": 1})
_win("fused_batched-more_units_than_compute_units", "k_xe_i8_fused", "i8", (64, 256, 32, 1), 20, _NL,
     {"windows": 20, "launches": 1, "all": lambda r: r["workgroups"] * r["units_per_workgroup"] > torch.cuda.get_device_properties(0).multi_processor_count})
_win("whole_line", "k_xe_i8_lines", "i8", (64, 64, 32, 1), 3, _LN, {"windows": 3, "launches": 1})
for _spg in (32, 8):
    _win("group_major", "k_xe_i8_fused", "i8", (64, 128, 64, 1), 3, want={"windows": 3, "launches": 1}, spg=_spg)
# 5 windows of 1024 channels = 4 (the whole-line kernel) + 1 (the fused kernel): the route keeps the last launch and the count of launches
_win("split_into_launches", "k_xe_i8_fused", "i8", (64, 1024, 32, 1), 5, want={"all": lambda r: r["launches"] >= 2, "windows": 1})
_win("window_loop-k_xe_pad_rows8", "k_xe_f32_fused+k_xe_reduce", "cf32", (9, 5, 33, 2), 2, want={"launches": 2})
_win("window_loop", "k_xe_turn+k_xe_corr", "p4", (5, 6, 70, 2), 2, want={"launches": 2})


@gpu_test
@pytest.mark.parametrize("label,kind,geo,nint,env,want,spg", WIN)
def test_windows_in_one_call_stay_inside_their_buffers(gpu, oracle, monkeypatch, label, kind, geo, nint, env, want, spg):
    """xcorrelate_n_device: nint windows in ONE guarded input and ONE guarded output.  The oracle's windows (and channel slices, see _data)
    are compared as always; every int8 window is also compared bit for bit with a one-window call on plain buffers."""
    _setenv(monkeypatch, env)
    N, F, T, npol = geo
    x, refs = _data(oracle, kind, N, F, T, npol, nint)
    blk = _block(gpu, kind, N, F, T, npol)
    per, nb = blk.get_output_buffer_size(), _nb(N, npol)
    if spg:  # [window][t][group][station] -> [group][window][t][station in group]
        xin = np.ascontiguousarray(x.reshape(nint, T, N // spg, spg, F, npol * 2).transpose(2, 0, 1, 3, 4, 5)).reshape(-1)
    else:
        xin = x.reshape(-1)
    payload = xin.view(np.int8) if kind == "p4" else xin
    plain = None
    if kind == "i8":
        plain = []
        for i in range(nint):
            y = torch.full((per,), float("nan"), dtype=torch.complex64, device=DEV)
            blk.xcorrelate_device(torch.from_numpy(x[i]).to(DEV), y)
            plain.append(to_numpy(y).view(np.uint32))
        torch.cuda.synchronize()

    def call(i, o):
        blk.xcorrelate_n_device(nint, i[0], o[0], stations_per_group=spg)
        _route(blk, label, want)

    def check(outs):
        got = outs[0].reshape(nint, F, nb)
        for i, f0, f1, r in refs:
            if kind == "i8":
                assert np.array_equal(got[i, f0:f1].reshape(-1).view(np.uint32), r.view(np.uint32)), (i, f0, f1)
            else:
                err = relerr(got[i, f0:f1].reshape(-1), r)
                print("relerr %s %s window %d %.3g" % (label, geo, i, err))
                assert err <= TOL, i
        if plain:
            for i in range(nint):
                assert np.array_equal(got[i].reshape(-1).view(np.uint32), plain[i]), "window %d differs from the one-window call" % i

    _run_offsets(call, [(payload, x[0].size // T)], [(nint * per, np.complex64, nb)], OUT2, check, bitwise=(kind == "i8"))
    blk.stop()


# ------------------------------------------------------------------------------------------------------------ sharded engine

@gpu_test
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
def test_sharded_submit_device_stays_inside_every_ranks_buffers(gpu, oracle, acc):
    """four ranks on one device, two windows: every rank's frames [window][t][station in group][channel] and its slab output
    [window][channel of the slab][baseline] guarded; the slab outputs 0 and 1 item past a 16-byte boundary"""
    W, N, F, T, windows = 4, 64, 256, 32, 2
    x, refs = _data(oracle, "i8", N, F, T, 1, windows)
    assert [(i, f0, f1) for i, f0, f1, _ in refs] == [(0, 0, F), (1, 0, F)]
    full = x.reshape(windows, T, N, F, 2)
    nb = _nb(N, 1)
    prior = _prior("i8", N, windows * F, 1).reshape(windows, F, nb)
    want = [(_with_prior(oracle, "i8", N, F, T, 1, x[w], prior[w].reshape(-1)) if acc else refs[w][3]).reshape(F, nb) for w in range(windows)]
    sh = gpu.clXEngineSharded([0] * W, 1, N, F, T, windows)
    Ng, Fw, slab = N // W, F // W, sh.slab_items()
    assert slab == Fw * nb
    for oo in (0, 1):
        fr = [guarded_input(np.ascontiguousarray(full[:, :, r * Ng:(r + 1) * Ng]), pad_items(1, Ng * F * 2), 0, DEV) for r in range(W)]
        out = [guarded_output(windows * slab, np.complex64, pad_items(8, nb), oo, DEV) for r in range(W)]
        assert all(v.numel() == sh.frames_bytes() and v.data_ptr() % 16 == 0 for _, v in fr)
        if acc:
            for r, (_, v) in enumerate(out):
                prefill_output(v, prior[:, r * Fw:(r + 1) * Fw])
        torch.cuda.synchronize()
        sh.submit_device([v for _, v in fr], [v for _, v in out], accumulate=acc)
        sh.synchronize()
        torch.cuda.synchronize()
        for r in range(W):
            check_guards(*fr[r], "frames of rank %d" % r)
            check_guards(*out[r], "slab output of rank %d at offset %d" % (r, oo))
            got = to_numpy(out[r][1]).reshape(windows, Fw, nb)
            for w in range(windows):
                assert np.array_equal(got[w].view(np.uint32), want[w][r * Fw:(r + 1) * Fw].view(np.uint32)), (oo, r, w)
    sh.close()


# ------------------------------------------------------------------------------------------------------------- pack3d_device

@gpu_test
@pytest.mark.parametrize("width,src_pitch,dst_pitch,gap", [(13, 29, 17, 3), (20, 32, 24, 4), (48, 64, 80, 16)],
                         ids=["bytes-width_13", "4_byte_units-width_20", "16_byte_units-width_48"])
def test_pack3d_device_stays_inside_its_buffers(gpu, width, src_pitch, dst_pitch, gap):
    """three blocks of five rows, pitches larger than the width, block strides larger than the rows: the rows land where they belong, the gaps
    between rows and blocks of the destination keep their pre-fill, nothing outside either buffer is touched.  The copy works in 16-byte,
    4-byte or 1-byte units, whichever all of the pointers, the width, the pitches and the strides allow: one case each."""
    rows, nblocks = 5, 3
    sblock, dblock = rows * src_pitch + gap, rows * dst_pitch + 2 * gap
    nsrc = (nblocks - 1) * sblock + (rows - 1) * src_pitch + width
    ndst = (nblocks - 1) * dblock + (rows - 1) * dst_pitch + width
    src = np.random.default_rng(width).integers(-128, 128, nsrc, dtype=np.int64).astype(np.int8)
    blk = _block(gpu, "i8", 8, 16, 32, 1)
    sw, sv = guarded_input(src, pad_items(1), 0, DEV)
    dw, dv = guarded_output(ndst, np.int8, pad_items(1), 0, DEV)
    want = to_numpy(dv).copy()
    for b in range(nblocks):
        for r in range(rows):
            want[b * dblock + r * dst_pitch:b * dblock + r * dst_pitch + width] = src[b * sblock + r * src_pitch:b * sblock + r * src_pitch + width]
    blk.pack3d_device(dv, sv, width, rows, nblocks, src_pitch, sblock, dst_pitch, dblock)
    torch.cuda.synchronize()
    check_guards(sw, sv, "source")
    check_guards(dw, dv, "destination", interior=False)
    assert np.array_equal(to_numpy(dv), want)
    blk.stop()


@gpu_test
def test_pack3d_device_refuses_short_tensors(gpu):
    """a tensor shorter than the extent the pitches and strides imply is a ValueError, and nothing is launched"""
    blk = _block(gpu, "i8", 8, 16, 32, 1)
    width, rows, nblocks, sp, sb, dp, db = 20, 5, 3, 32, 164, 24, 128
    nsrc, ndst = 2 * sb + 4 * sp + width, 2 * db + 4 * dp + width
    src = torch.ones(nsrc, dtype=torch.int8, device=DEV)
    dst = torch.zeros(ndst, dtype=torch.int8, device=DEV)
    with pytest.raises(ValueError, match="source"):
        blk.pack3d_device(dst, src[:-1], width, rows, nblocks, sp, sb, dp, db)
    with pytest.raises(ValueError, match="destination"):
        blk.pack3d_device(dst[:-1], src, width, rows, nblocks, sp, sb, dp, db)
    torch.cuda.synchronize()
    assert not dst.any(), "a refused call wrote its destination"
    blk.pack3d_device(dst, src, width, rows, nblocks, sp, sb, dp, db)  # exactly the extent: accepted
    torch.cuda.synchronize()
    assert int(dst.sum()) == width * rows * nblocks
    blk.stop()


# ------------------------------------------------------------------------------------------------ host calls: the copy back

@gpu_test
@pytest.mark.parametrize("path", ["xcorrelate", "submit_wait", "sharded_xcorrelate", "sharded_wait"])
def test_host_calls_write_the_output_items_and_nothing_else(gpu, oracle, path):
    """numpy outputs as views into larger sentinel-filled arrays (the pattern of test_device_bounds_gpu._host_out)"""
    sharded = path.startswith("sharded")
    N, F, T = (16, 64, 64) if sharded else (20, 64, 33)
    x, refs = _data(oracle, "i8", N, F, T, 1)
    n = F * _nb(N, 1)
    whole, view, lo = _host_out(n, np.complex64)
    if path == "xcorrelate":
        blk = _block(gpu, "i8", N, F, T, 1)
        blk.xcorrelate(x[0], view)
        blk.stop()
    elif path == "submit_wait":
        blk = _block(gpu, "i8", N, F, T, 1)
        blk.submit(x[0])
        blk.wait(view)
        blk.stop()
    else:
        sh = gpu.clXEngineSharded([0, 0], 1, N, F, T, 1)
        if path == "sharded_xcorrelate":
            sh.xcorrelate(x[0], view)
        else:
            sh.acquire()[:] = x[0]
            sh.submit_acquired()
            sh.wait(view)
        sh.close()
    _host_check(whole, lo, n)
    assert np.array_equal(view.view(np.uint32), refs[0][3].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- the inventory (CPU)

def test_every_route_label_is_accounted_for():
    """every string literal in the first argument of a mi355_xe_route_set(...) call of csrc/xengine*.hip is a row of ROUTES, and every
    row of ROUTES is the asserted route of at least one guarded case above: a route added later cannot be forgotten here"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "gr-clenabled_amd", "csrc", "xengine*.hip")))
    assert len(files) >= 4, files
    found = set()
    for path in files:
        with open(path) as f:
            text = f.read()
        for m in re.finditer(r"(?<!void )mi355_xe_route_set\(([^;{]*?)\);", text):
            labels = re.findall(r"\"([^\"]+)\"", m.group(1))
            assert labels, "a route label that is not a string literal: %s" % m.group(0)
            found.update(labels)
    assert found, "no mi355_xe_route_set call found"
    assert found - set(ROUTES) == set(), "routes without a row in ROUTES (and a guarded case): %s" % sorted(found - set(ROUTES))
    assert set(ROUTES) - found == set(), "rows of ROUTES the library no longer records: %s" % sorted(set(ROUTES) - found)
    assert set(ROUTES) - ASSERTED == set(), "routes no guarded case asserts: %s" % sorted(set(ROUTES) - ASSERTED)
