"""clFilterbankCleaner without a device: the yardstick tests/fbclean_ref.py against hand-worked tiny cases (a NaN column, a constant column,
a masked channel, no good channel at all, a time sample exactly on the td boundary), the proof that a sequential sum is another function
than the contract's segment tree, mi355_fbclean_sk_estimate against the yardstick bit for bit, the sizes of mi355_fbclean_plan, every
argument error of _plan / _create with a NULL context (which shows that the arguments are checked before the context is touched), NULL
handles, the library's exports against the header, and the end-to-end fixture validated with the references alone.  The kernels are
tested in tests/test_fbclean_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import fbclean_ref as ref

NAMES = {"plan", "create", "destroy", "set_limits", "get_limits", "set_mask", "get_mask", "block_len", "set_generic", "route", "work", "work_dev",
         "sk_estimate"}
INF = float("inf")


def _plan(L, R, F, Tb):
    a, b, c = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    rc = L.mi355_fbclean_plan(R, F, Tb, C.byref(a), C.byref(b), C.byref(c))
    return rc, (a.value, b.value, c.value), L.mi355_last_error().decode()


def _create(L, R, F, Tb, nd=1.0, sk_lo=-INF, sk_hi=INF, td=INF, zero_dm=0, ctx=None):
    h = C.c_void_p(1)
    rc = L.mi355_fbclean_create(ctx, R, F, Tb, nd, sk_lo, sk_hi, td, zero_dm, None, C.byref(h))
    assert rc != 0 and not h.value  # no handle comes back from a refused create
    return rc, L.mi355_last_error().decode()


def test_header_symbols_are_exported(pkg):
    """every mi355_fbclean_* function the header declares is in the library, and they are the thirteen of the contract"""
    with open(os.path.join(ROOT, "include", "mi355_clenabled.h")) as f:
        declared = set(re.findall(r"^[a-z][a-z ]*\*?\b(mi355_fbclean_\w+)\(", f.read(), re.M))
    assert declared == {"mi355_fbclean_" + n for n in NAMES} and len(declared) == 13
    L = pkg.lib()
    for name in sorted(declared):
        assert getattr(L, name) is not None, name


def test_plan_sizes(pkg):
    L = pkg.lib()
    for R, F, Tb in ((64, 1024, 256), (1, 1, 16), (3, 52, 48), (4096, 16384, 4096)):
        assert _plan(L, R, F, Tb)[:2] == (0, ref.plan(R, F))
    assert _plan(L, 64, 1024, 256)[1] == (65536, 65536, 64)
    assert L.mi355_fbclean_plan(2, 8, 16, None, None, None) == 0  # any output pointer may be NULL


BAD_SHAPE = [
    ((0, 8, 16), "num_rows must be 1 .. 4096"),
    ((4097, 8, 16), "num_rows must be 1 .. 4096"),
    ((2, 0, 16), "num_channels must be 1 .. 16384"),
    ((2, 16385, 16), "num_channels must be 1 .. 16384"),
    ((2, 8, 0), "block_len must be a multiple of 16 in 16 .. 4096"),
    ((2, 8, 15), "block_len must be a multiple of 16 in 16 .. 4096"),
    ((2, 8, 40), "block_len must be a multiple of 16 in 16 .. 4096"),
    ((2, 8, 4112), "block_len must be a multiple of 16 in 16 .. 4096"),
]


@pytest.mark.parametrize("args,msg", BAD_SHAPE)
def test_shape_errors_come_before_the_context(pkg, args, msg):
    L = pkg.lib()
    assert _plan(L, *args) == (-1, (0, 0, 0), "invalid argument: " + msg)
    assert _create(L, *args) == (-1, "invalid argument: " + msg)                              # NULL context
    assert _create(L, *args, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: " + msg)  # an invalid one is never touched


BAD_LIMITS = [
    (dict(nd=0.0), "nd must be positive and finite"),
    (dict(nd=-1.0), "nd must be positive and finite"),
    (dict(nd=INF), "nd must be positive and finite"),
    (dict(nd=float("nan")), "nd must be positive and finite"),
    (dict(sk_lo=1.5, sk_hi=1.0), "sk_lo must not be above sk_hi (NaN is refused)"),
    (dict(sk_lo=float("nan")), "sk_lo must not be above sk_hi (NaN is refused)"),
    (dict(sk_hi=float("nan")), "sk_lo must not be above sk_hi (NaN is refused)"),
    (dict(td=-0.5), "td must be >= 0 (NaN is refused)"),
    (dict(td=float("nan")), "td must be >= 0 (NaN is refused)"),
    (dict(zero_dm=2), "zero_dm must be 0 or 1"),
    (dict(zero_dm=-1), "zero_dm must be 0 or 1"),
]


@pytest.mark.parametrize("kw,msg", BAD_LIMITS)
def test_limit_errors_come_before_the_context(pkg, kw, msg):
    L = pkg.lib()
    assert _create(L, 2, 8, 16, **kw) == (-1, "invalid argument: " + msg)
    assert _create(L, 2, 8, 16, ctx=C.c_void_p(0xDEAD0000), **kw) == (-1, "invalid argument: " + msg)


def test_create_checks_the_arguments_then_the_context(pkg):
    L = pkg.lib()
    assert _create(L, 2, 8, 16) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert _create(L, 4096, 16384, 4096, 16.0, 0.5, 1.5, 0.0, 1) == (-1, "invalid argument: NULL context")
    assert _create(L, 2, 8, 16, sk_lo=1.0, sk_hi=1.0) == (-1, "invalid argument: NULL context")  # sk_lo == sk_hi is in order
    assert L.mi355_fbclean_create(None, 2, 8, 16, 1.0, -INF, INF, INF, 0, None, None) == -1


def test_null_handles(pkg):
    L = pkg.lib()
    assert L.mi355_fbclean_set_limits(None, 1.0, -INF, INF, INF, 0) == -1 and L.mi355_fbclean_get_limits(None, None, None, None, None, None) == -1
    assert L.mi355_fbclean_set_mask(None, None) == -1 and L.mi355_fbclean_get_mask(None, None, 0) == -1
    assert L.mi355_fbclean_set_generic(None, 1) == -1 and L.mi355_fbclean_block_len(None) == -1
    assert L.mi355_fbclean_work(None, 16, None, None, None, None, None) == -1
    assert L.mi355_fbclean_work_dev(None, 16, None, None, None, None, None, None) == -1
    assert L.mi355_fbclean_route(None) == b"" and L.mi355_fbclean_destroy(None) == 0


def test_python_class_refuses_before_a_context_exists(pkg):
    with pytest.raises(pkg.Mi355Error):
        pkg.clFilterbankCleaner(1, 2, 0, 99, 2, 8, 40)  # block_len; device 99 is never looked for
    with pytest.raises(ValueError):
        pkg.clFilterbankCleaner(1, 2, 0, 99, 2, 8, 16, mask=np.zeros(5, np.uint8))
    with pytest.raises(TypeError):
        pkg.clFilterbankCleaner(1, 2, 0, 99, 2, 8, 16, mask=np.zeros(8, np.int32))


def _alt(a, b, n=16):
    return np.tile(np.array([a, b], np.float32), n // 2)


def _five():
    """Tb = 16 (segments of one sample), R = 1, F = 5: f0 = 1, 3, 1, 3 ... (m 2, var 1), f1 the same with a NaN, f2 constant, f3 = 10, 20,
    ... (m 15, var 25), f4 = 0, 4, ... (m 2, var 4)"""
    x = np.empty((16, 1, 5), np.float32)
    x[:, 0, 0] = _alt(1, 3)
    x[:, 0, 1] = _alt(1, 3)
    x[3, 0, 1] = np.nan
    x[:, 0, 2] = 7.0
    x[:, 0, 3] = _alt(10, 20)
    x[:, 0, 4] = _alt(0, 4)
    return x


def test_ref_hand_worked_flags_and_normalisation():
    x = _five()
    mask = np.array([0, 0, 0, 1, 0], np.uint8)
    out, cf, tf, st = ref.clean(x, 16, 1.0, mask=mask)
    assert cf.tolist() == [[[0, 1, 1, 1, 0]]] and not tf.any()
    # {m32, is32} wherever var > 0, the masked channel included; {0, 0} for the NaN column and the constant one
    assert st[0, 0].tolist() == [[2.0, 1.0], [0.0, 0.0], [0.0, 0.0], [15.0, float(np.float32(0.2))], [2.0, 0.5]]
    assert np.array_equal(out[:, 0, 0], _alt(-1, 1)) and np.array_equal(out[:, 0, 4], _alt(-1, 1))
    for f in (1, 2, 3):
        assert not out[:, 0, f].any() and not np.signbit(out[:, 0, f]).any()  # +0.0f
    # sk = ((M nd + 1) / (M - 1)) ((M s2) / (s1 s1) - 1): f0 s1 = 32, s2 = 80: 17/15 * 0.25; f4 s1 = 32, s2 = 128: 17/15 * 1
    assert ref.sk_estimate(x[:, 0, 0], 1.0) == (17.0 / 15.0) * 0.25 and ref.sk_estimate(x[:, 0, 4], 1.0) == 17.0 / 15.0
    assert ref.sk_estimate(x[:, 0, 3], 3.0) == (49.0 / 15.0) * ((16.0 * 4000.0) / (240.0 * 240.0) - 1.0)
    # the limits are inclusive, and each side flags on its own (f3: sk = 17/15 * 0.111 is below lo)
    lo, hi = (17.0 / 15.0) * 0.25, 17.0 / 15.0
    assert ref.clean(x, 16, 1.0, lo, hi)[1].tolist() == [[[0, 1, 1, 1, 0]]]
    assert ref.clean(x, 16, 1.0, np.nextafter(lo, 1), hi)[1].tolist() == [[[1, 1, 1, 1, 0]]]
    assert ref.clean(x, 16, 1.0, lo, np.nextafter(hi, 0))[1].tolist() == [[[0, 1, 1, 1, 1]]]


def test_ref_hand_worked_zero_dm():
    x = _five()
    x[:, 0, 4] = _alt(4, 0)  # the opposite phase: y = +1, -1, ...
    # good: f0 (-1, +1, ...), f3 (-1, +1, ...), f4 (+1, -1, ...): zs = -1, +1, ...; ng = 3
    out, cf, tf, st = ref.clean(x, 16, 1.0, zero_dm=1)
    assert cf.tolist() == [[[0, 1, 1, 0, 0]]] and not tf.any()
    third = np.float32(1.0 / 3.0)
    assert np.array_equal(out[:, 0, 0], _alt(np.float32(-1) + third, np.float32(1) - third))
    assert np.array_equal(out[:, 0, 3], out[:, 0, 0])
    assert np.array_equal(out[:, 0, 4], _alt(np.float32(1) + third, np.float32(-1) - third))
    assert not out[:, 0, 1:3].any() and not np.signbit(out[:, 0, 1:3]).any()
    # zs zs = 1 > td2 ng = 3 td td for td < 1 / sqrt(3): every time sample flagged, everything +0.0f
    out, cf, tf, st = ref.clean(x, 16, 1.0, td=0.5, zero_dm=1)
    assert tf.all() and not out.any() and not np.signbit(out).any() and cf.tolist() == [[[0, 1, 1, 0, 0]]]
    # with zero_dm off the same td flags nothing and y' = y
    out, cf, tf, st = ref.clean(x, 16, 1.0, td=0.5, zero_dm=0)
    assert not tf.any() and np.array_equal(out[:, 0, 4], _alt(1, -1))


def test_ref_td_boundary_and_no_good_channel():
    x = _five()
    x[3, 0, 1] = 3.0  # no NaN any more: f0, f1, f3, f4 good and in phase, zs = -4, +4, ...; ng = 4; zs zs = 16
    out, cf, tf, st = ref.clean(x, 16, 1.0, td=2.0, zero_dm=1)
    assert cf.tolist() == [[[0, 0, 1, 0, 0]]]
    assert not tf.any()  # 16 > 2 * 2 * 4 is false: exactly on the boundary is not flagged
    assert not out.any()  # and y - z32 = -1 - (-1) = +0
    out, cf, tf, st = ref.clean(x, 16, 1.0, td=np.nextafter(2.0, 0.0), zero_dm=1)
    assert tf.all() and not out.any()
    # no good channel at all: ng = 0, zs = 0, 0 > td2 0 is false (and NaN for td = Inf: false as well); z32 = NaN reaches nothing
    for td in (0.0, 2.0, np.inf):
        out, cf, tf, st = ref.clean(x, 16, 1.0, td=td, zero_dm=1, mask=np.ones(5, np.uint8))
        assert cf.all() and not tf.any() and not out.any() and not np.signbit(out).any()
        assert st[0, 0, 0].tolist() == [2.0, 1.0]  # the statistics of a masked channel are still reported


def test_ref_nan_and_inf_reach_one_cell():
    rng = np.random.default_rng(4)
    x = ref.gamma(rng, 64, 2, 6)
    base = ref.clean(x, 32, 16.0)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[40, 1, 2] = bad
        out, cf, tf, st = ref.clean(y, 32, 16.0)
        assert cf[1, 1, 2] == 1 and cf.sum() == 1 and st[1, 1, 2].tolist() == [0.0, 0.0]
        assert not out[32:, 1, 2].any()
        keep = np.ones(x.shape, bool)
        keep[32:, 1, 2] = False
        assert np.array_equal(out[keep], base[0][keep]) and not np.isnan(out).any()


def test_a_sequential_sum_is_not_the_tree():
    """the contract is 16 sequential segments and a tree over them: a plain sequential float64 sum has other bits"""
    rng = np.random.default_rng(1)
    x = ref.gamma(rng, 256, 2, 64)
    s1, s2 = ref.block_sums(x)
    q1, q2 = ref.sequential_sums(x)
    assert np.mean(s2 != q2) > 0.9 and np.allclose(s2, q2, rtol=1e-13)
    w = ref.wide_range(rng, 256, 2, 64)
    s1, s2 = ref.block_sums(w)
    q1, q2 = ref.sequential_sums(w)
    assert np.mean(s1 != q1) > 0.5 and np.allclose(s1, q1, rtol=1e-13)


@pytest.mark.parametrize("Tb", [16, 48, 256, 4096])
def test_sk_estimate_is_the_reference_bit_for_bit(pkg, Tb):
    rng = np.random.default_rng(Tb)
    x = ref.gamma(rng, Tb, 2, 3)
    w = ref.wide_range(rng, Tb, 2, 3)
    for a in (x, w):
        flat = a.reshape(Tb, 6)
        for col in range(6):
            for nd in (1.0, 16.0, 2.5):
                want = ref.sk_estimate(flat[:, col], nd)
                assert pkg.sk_estimate(np.ascontiguousarray(flat[:, col]), nd) == want
                assert pkg.sk_estimate(flat.reshape(-1)[col:], nd, stride=6) == want
    const = np.full(Tb, 3.0, np.float32)
    assert pkg.sk_estimate(const, 1.0) == ref.sk_estimate(const, 1.0)
    assert np.isnan(pkg.sk_estimate(np.zeros(Tb, np.float32), 1.0))


def test_sk_estimate_refuses_bad_arguments(pkg):
    L = pkg.lib()
    x = np.ones(64, np.float32)
    sk = C.c_double()
    p = C.c_void_p(x.ctypes.data)
    assert L.mi355_fbclean_sk_estimate(None, 16, 1, 1.0, C.byref(sk)) == -1 and L.mi355_fbclean_sk_estimate(p, 16, 1, 1.0, None) == -1
    assert L.mi355_fbclean_sk_estimate(p, 24, 1, 1.0, C.byref(sk)) == -1 and L.mi355_fbclean_sk_estimate(p, 16, 0, 1.0, C.byref(sk)) == -1
    assert L.mi355_fbclean_sk_estimate(p, 16, 1, 0.0, C.byref(sk)) == -1 and L.mi355_fbclean_sk_estimate(p, 16, 4, 1.0, C.byref(sk)) == 0


def test_ref_search_scene_cleaning_moves_the_peak_from_the_spike_to_the_pulse():
    """the end-to-end fixture of tests/test_fbclean_gpu.py with the references alone (fbclean_ref -> dedisp_ref -> psearch_ref)"""
    sc = ref.search_scene()
    D, Tb = sc["D"], sc["Tb"]
    # without cleaning the strongest record lies at the zero-DM spike
    pk = ref.search(sc, sc["x"])
    b, s = np.unravel_index(np.argmax(pk["snr"]), pk.shape)
    k, t = int(pk["loc"][b, s]) >> 24, b * Tb + (int(pk["loc"][b, s]) & 0xFFFFFF)
    assert s // D == sc["r0"] and t <= sc["t_spike"] and sc["t_spike"] + 4 <= t + (1 << k) + int(sc["tab"][s % D].max())
    assert s % D != sc["d0"] or abs(t - sc["t0"]) > 16
    # with it, at the pulse's trial and time, width 8
    out, cf, tf, st = ref.clean(sc["x"], Tb, sc["nd"], sc["sk_lo"], sc["sk_hi"], sc["td"], 1)
    pk = ref.search(sc, out)
    b, s = np.unravel_index(np.argmax(pk["snr"]), pk.shape)
    assert (s, b) == (sc["r0"] * D + sc["d0"], sc["t0"] // Tb) and pk["loc"][b, s] == (3 << 24) | (sc["t0"] % Tb)
    assert 30 < pk["snr"][b, s] < 50 and np.sort(pk["snr"].reshape(-1))[-2] < pk["snr"][b, s] - 3
    # the bursty channel is flagged in every block of both rows, the spike's time samples are flagged in its row and no others
    assert cf[:, :, sc["f_bad"]].all()
    assert np.argwhere(tf).tolist() == [[sc["t_spike"] + i, sc["r0"]] for i in range(4)]
    clean_cells = np.delete(cf, sc["f_bad"], axis=2)
    assert clean_cells.mean() <= 0.02
