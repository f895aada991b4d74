"""clFolder without a device: the library's exports against the header, mi355_fold_bins against the yardstick tests/fold_ref.py bit for
bit (wrap-around near 2^63 and 2^64, negative nudot, nbin 2, 3, 1000, 4096, nu = 0, a period below two samples), mi355_fold_model
against exact rational arithmetic within its stated rounding (two units), the sizes of mi355_fold_plan, every shape error of _plan / _create with
a NULL context (which shows that the arguments are checked before the context is touched), NULL handles, hand-worked tiny folds of the
yardstick, and the proof that a pairwise tree is another function than the contract's sum.  The kernels are tested in
tests/test_fold_gpu.py."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
import fold_ref as ref

NAMES = {"plan", "create", "destroy", "set_models", "get_models", "sample", "set_sample", "skip", "subint_len", "set_generic", "route", "work",
         "work_dev", "model", "bins"}
M64 = (1 << 64) - 1


def _plan(L, R, F, nbin, Ts):
    a, b, c = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    rc = L.mi355_fold_plan(R, F, nbin, Ts, C.byref(a), C.byref(b), C.byref(c))
    return rc, (a.value, b.value, c.value), L.mi355_last_error().decode()


def _create(L, R, F, nbin, Ts, ctx=None):
    h = C.c_void_p(1)
    m = np.zeros(3 * max(R, 1), np.uint64)
    rc = L.mi355_fold_create(ctx, R, F, nbin, Ts, C.c_void_p(m.ctypes.data), C.byref(h))
    assert rc != 0 and not h.value  # no handle comes back from a refused create
    return rc, L.mi355_last_error().decode()


def test_header_symbols_are_exported(pkg):
    """every mi355_fold_* function the header declares is in the library, and they are the fifteen of the contract"""
    with open(os.path.join(ROOT, "include", "mi355_clenabled.h")) as f:
        declared = set(re.findall(r"^[a-z][a-z ]*\*?\b(mi355_fold_\w+)\(", f.read(), re.M))
    assert declared == {"mi355_fold_" + n for n in NAMES} and len(declared) == 15
    L = pkg.lib()
    for name in sorted(declared):
        assert getattr(L, name) is not None, name
    assert callable(pkg.fold_model) and callable(pkg.fold_bins) and pkg.clFolder.fold_bins is pkg.fold_bins


BIN_CASES = [
    # (phi0, nu, nudot, T0, n, nbin)
    (0, 1 << 60, 0, 0, 64, 16),                                       # 16 samples per turn
    (0x123456789ABCDEF0, 0x0123456789ABCDEF, 0, (1 << 63) - 20, 48, 3),   # T crosses 2^63: nu T wraps many times
    (5, 0xFEDCBA9876543210, -12345678901234567, (1 << 63) - 7, 40, 1000), # negative nudot, a period below two samples
    (0, (1 << 64) // 7, 3 << 40, (1 << 40) - 5, 64, 4096),
    (1 << 63, 0, 0, 12345, 32, 2),                                    # nu = 0: everything in one bin
    (0, 0, 1 << 58, 0, 64, 7),                                        # the phase moves by nudot alone
    (77, (1 << 64) // 3 + 1, -(1 << 50) - 1, M64 - 20, 48, 3),            # T itself wraps to 0 inside the run
    (0, (1 << 63) + 12345, 1, M64 - 3, 16, 4096),
]


@pytest.mark.parametrize("phi0,nu,nudot,T0,n,nbin", BIN_CASES)
def test_fold_bins_equals_the_yardstick(pkg, phi0, nu, nudot, T0, n, nbin):
    m = ref.words(phi0, nu, nudot)
    want = ref.bins(m, T0, n, nbin)
    got = pkg.fold_bins(m, T0, n, nbin)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert want.min() >= 0 and want.max() < nbin
    if nu == 0 and nudot == 0:
        assert len(set(want.tolist())) == 1


def test_fold_bins_hand_worked(pkg):
    """nu = 2^62 is a period of four samples: with four bins the bin is T mod 4; tri() is T (T - 1) / 2"""
    assert pkg.fold_bins(ref.words(0, 1 << 62, 0), 0, 8, 4).tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert pkg.fold_bins(ref.words(1 << 63, 1 << 62, 0), 1, 4, 4).tolist() == [3, 0, 1, 2]
    assert [ref.tri(T) for T in range(7)] == [0, 0, 1, 3, 6, 10, 15]
    assert pkg.fold_bins(ref.words(0, 0, 1 << 61), 0, 6, 8).tolist() == [0, 0, 1, 3, 6, 2]   # tri(T) mod 8
    # T wraps: T = 2^64 - 1, then 0
    assert ref.tri(M64) == ((M64 * (M64 - 1)) // 2) & M64
    assert pkg.fold_bins(ref.words(0, 1 << 62, 0), M64, 2, 4).tolist() == [3, 0]


def test_fold_bins_and_model_refuse(pkg):
    L = pkg.lib()
    m = ref.words(0, 1, 0)
    out = np.zeros(4, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert L.mi355_fold_bins(None, 0, 4, 8, p(out)) == -1
    assert L.mi355_fold_bins(p(m), 0, -1, 8, p(out)) == -1
    assert L.mi355_fold_bins(p(m), 0, 4, 1, p(out)) == -1 and L.mi355_fold_bins(p(m), 0, 4, 4097, p(out)) == -1
    assert L.mi355_fold_bins(p(m), 0, 4, 8, None) == -1 and L.mi355_fold_bins(p(m), 0, 0, 8, None) == 0
    w = np.zeros(3, np.uint64)
    for bad in ((0.0, 0.0, 1e-3, 0.0), (-1.0, 0.0, 1e-3, 0.0), (1.0, 0.0, 0.0, 0.0), (1.0, 0.0, -1e-3, 0.0), (float("nan"), 0.0, 1e-3, 0.0),
                (1.0, float("inf"), 1e-3, 0.0), (1.0, 0.0, float("inf"), 0.0), (1.0, 0.0, 1e-3, float("nan")), (1.0, 1.0, 1.0, 0.0)):
        assert L.mi355_fold_model(*bad, p(w)) == -1, bad
    assert L.mi355_fold_model(1.0, 0.0, 1e-3, 0.0, None) == -1


MODEL_CASES = [(0.033, 4.2e-13, 64e-6, 0.25), (1.337, 0.0, 1e-3, 0.0), (0.00557, -1e-19, 81.92e-6, -0.125), (1.5e-3, 0.0, 1e-3, 3.75),
               (0.7, 1e-6, 0.01, 0.5)]


@pytest.mark.parametrize("period,pdot,tsamp,phase0", MODEL_CASES)
def test_fold_model_is_within_two_units(pkg, period, pdot, tsamp, phase0):
    """the stated rounding: each word within two units of 2^-64 of the exact value of the contract's formulas on the given doubles; a
    period then round-trips to within tsamp 2^-63 / nu^2 seconds (nu in turns per sample)"""
    w = [int(v) for v in pkg.fold_model(period, pdot, tsamp, phase0)]
    q = Fraction(tsamp) / Fraction(period)
    nd = -Fraction(pdot) * q * q
    two64 = 1 << 64
    exact = [(Fraction(phase0) % 1) * two64, ((q + nd / 2) % 1) * two64, nd * two64]
    signed = w[2] - two64 if w[2] >> 63 else w[2]
    for got, want in zip((w[0], w[1], signed), exact):
        err = abs(Fraction(got) - want)
        assert min(err, two64 - err) <= 2, (got, float(want))
    if pdot == 0.0 and q < 1:
        back = Fraction(tsamp) / (Fraction(w[1]) / two64)
        assert abs(back - Fraction(period)) <= 2 * Fraction(tsamp) * two64 / (Fraction(w[1]) ** 2) * Fraction(101, 100)


def test_plan_sizes(pkg):
    L = pkg.lib()
    assert _plan(L, 64, 1024, 256, 4096)[:2] == (0, (65536, 64 * 256 * 1024, 64 * 256))
    assert _plan(L, 1, 1, 2, 16)[:2] == (0, (1, 2, 2))
    assert _plan(L, 3, 52, 7, 48)[:2] == (0, (156, 3 * 7 * 52, 21))
    assert _plan(L, 4096, 16384, 4096, 16384)[:2] == (0, (4096 * 16384, 4096 * 4096 * 16384, 4096 * 4096))
    assert L.mi355_fold_plan(2, 8, 4, 16, None, None, None) == 0  # any output pointer may be NULL


BAD_SHAPE = [
    ((0, 8, 4, 16), "num_rows must be 1 .. 4096"),
    ((4097, 8, 4, 16), "num_rows must be 1 .. 4096"),
    ((2, 0, 4, 16), "num_channels must be 1 .. 16384"),
    ((2, 16385, 4, 16), "num_channels must be 1 .. 16384"),
    ((2, 8, 1, 16), "nbin must be 2 .. 4096"),
    ((2, 8, 4097, 16), "nbin must be 2 .. 4096"),
    ((2, 8, 4, 0), "subint_len must be a multiple of 16 in 16 .. 16384"),
    ((2, 8, 4, 15), "subint_len must be a multiple of 16 in 16 .. 16384"),
    ((2, 8, 4, 40), "subint_len must be a multiple of 16 in 16 .. 16384"),
    ((2, 8, 4, 16400), "subint_len must be a multiple of 16 in 16 .. 16384"),
]


@pytest.mark.parametrize("args,msg", BAD_SHAPE)
def test_shape_errors_come_before_the_context(pkg, args, msg):
    L = pkg.lib()
    assert _plan(L, *args) == (-1, (0, 0, 0), "invalid argument: " + msg)
    assert _create(L, *args) == (-1, "invalid argument: " + msg)                              # NULL context
    assert _create(L, *args, ctx=C.c_void_p(0xDEAD0000)) == (-1, "invalid argument: " + msg)  # an invalid one is never touched


def test_create_checks_the_arguments_then_the_context(pkg):
    L = pkg.lib()
    assert _create(L, 2, 8, 4, 16) == (-1, "invalid argument: NULL context")  # everything else was in order
    assert _create(L, 4096, 16384, 4096, 16384) == (-1, "invalid argument: NULL context")
    h = C.c_void_p(1)
    assert L.mi355_fold_create(None, 2, 8, 4, 16, None, C.byref(h)) == -1 and L.mi355_last_error() == b"invalid argument: models is NULL"
    assert L.mi355_fold_create(None, 2, 8, 4, 16, None, None) == -1


def test_null_handles(pkg):
    L = pkg.lib()
    assert L.mi355_fold_set_models(None, None) == -1 and L.mi355_fold_get_models(None, None, 0) == -1
    assert L.mi355_fold_sample(None, None) == -1 and L.mi355_fold_set_sample(None, 0) == -1 and L.mi355_fold_skip(None, 0) == -1
    assert L.mi355_fold_set_generic(None, 1) == -1 and L.mi355_fold_subint_len(None) == -1
    assert L.mi355_fold_work(None, 16, None, None, None, None) == -1
    assert L.mi355_fold_work_dev(None, 16, None, None, None, None, None) == -1
    assert L.mi355_fold_route(None) == b"" and L.mi355_fold_destroy(None) == 0


def test_yardstick_hand_worked():
    """a period of four samples into four bins over 16 samples: bin b holds x[b] + x[b + 4] + x[b + 8] + x[b + 12] in that order; a
    flagged sample leaves the sum and the hits; a NaN reaches its own (bin, channel) alone; -0.0f folds to +0.0f; an empty bin is +0.0f"""
    m = [ref.words(0, 1 << 62, 0)]
    x = np.arange(32, dtype=np.float32).reshape(16, 1, 2)
    out, hits = ref.fold(x, m, 0, 4, 16)
    assert out.shape == (1, 1, 4, 2) and np.array_equal(out[0, 0, :, 0], [48, 56, 64, 72]) and np.array_equal(hits[0, 0], [4, 4, 4, 4])
    tf = np.zeros((16, 1), np.uint8)
    tf[5, 0] = 1
    out, hits = ref.fold(x, m, 0, 4, 16, tf)
    assert np.array_equal(out[0, 0, :, 0], [48, 56 - 10, 64, 72]) and np.array_equal(hits[0, 0], [4, 3, 4, 4])
    out, hits = ref.fold(x, m, 2, 4, 16)           # the stream starts at T = 2: x[0] is in bin 2
    assert np.array_equal(out[0, 0, :, 0], [64, 72, 48, 56])
    y = x.copy()
    y[6, 0, 1] = np.nan
    out, _ = ref.fold(y, m, 0, 4, 16)
    assert np.isnan(out).sum() == 1 and np.isnan(out[0, 0, 2, 1])
    z = np.full((16, 1, 2), -0.0, np.float32)
    out, hits = ref.fold(z, m, 0, 8, 16)           # eight bins, a period of four samples: the odd bins stay empty
    assert np.array_equal(out.view(np.uint32), np.zeros(out.shape, np.uint32)) and np.array_equal(hits[0, 0], [4, 0, 4, 0, 4, 0, 4, 0])


def test_a_pairwise_tree_is_another_function():
    """the summation order is the contract: on a seeded input the adjacent-pair tree over the samples of one bin differs in bits from
    the sum in ascending time (which is why a tree reduction or a float atomic does not conform)"""
    rng = np.random.default_rng(20261021)
    nbin, Ts, F = 8, 1024, 16
    m = [ref.words(0, (1 << 64) // 8 + 12345678901, 0)]
    x = rng.gamma(4.0, 1.0, (Ts, 1, F)).astype(np.float32)
    out, hits = ref.fold(x, m, 0, nbin, Ts)
    b = ref.bins(m[0], 0, Ts, nbin)
    differing = 0
    for k in range(nbin):
        rows = x[b == k, 0, :]
        assert rows.shape[0] == hits[0, 0, k] and hits[0, 0, k] > 64
        tree = np.array([ref.pairwise(rows[:, f]) for f in range(F)], np.float32)
        seq = np.zeros(F, np.float32)
        for row in rows:
            seq = seq + row
        assert np.array_equal(seq.view(np.uint32), out[0, 0, k].view(np.uint32))
        assert np.allclose(tree, seq, rtol=1e-5)
        differing += int((tree.view(np.uint32) != seq.view(np.uint32)).sum())
    assert differing > 0
