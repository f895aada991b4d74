"""CPU: the yardsticks of the direct-form filters (tests/fir_ref.py) and of the channelizer (tests/pfb_ref.py) themselves -- the two forms
of each formula agree, float32 arithmetic in any order stays inside half of the bound, the bound is far tighter than the whole-call
metric it replaces (1e-5 max |ref|), and a planted loss of eight mantissa bits is caught by the bound though it passes the old metric.
Run with -s for the figures."""
import functools

import numpy as np
import pytest

import fir_ref as ref
import pfb_ref

OLD_TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _case(kernel, K, D, cplx):
    n = ref.nout(kernel, K, D)
    h = ref.make_taps(K, cplx)
    x = ref.make_input(K, D, n)
    want = ref.fir(h, x, D, n)
    bnd = ref.bound(h, x, D, n)
    return n, h, x, want, bnd


def _id(c):
    return "%s-%d-%d%s" % (c[0], c[1], c[2], "-c" if c[3] else "")


@pytest.mark.parametrize("case", ref.cases(), ids=_id)
def test_two_forms_agree(case):
    n, h, x, want, bnd = _case(*case)
    other = ref.fir_by_convolve(h, x, case[2], n)
    assert np.abs(other - want).max() <= 1e-12 * np.abs(want).max() * max(case[1], 8)


@pytest.mark.parametrize("case", ref.cases(), ids=_id)
def test_float32_orders_use_at_most_half_of_the_bound(case):
    n, h, x, want, bnd = _case(*case)
    for name, y in ref.float32_orders(h, x, case[2], n).items():
        r = ref.worst(y, want, bnd)
        print("%-28s float32 %-8s worst error / bound %.3f" % (_id(case), name, r))
        assert r <= 0.5, (name, r)


@pytest.mark.parametrize("case", ref.cases(), ids=_id)
def test_bound_is_not_vacuous(case):
    """the median per-output bound against the old form 1e-5 max |ref|: at least 5 times smaller up to 128 taps, never larger"""
    n, h, x, want, bnd = _case(*case)
    old = OLD_TOL * np.abs(want).max()
    med = float(np.median(bnd))
    print("%-28s median bound %.3g, largest %.3g, old form %.3g: old / median %.1f" % (_id(case), med, bnd.max(), old, old / med))
    assert med <= old
    if case[1] <= 128:
        assert 5.0 * med <= old


def _planted(mutate):
    K, D, n = 65, 1, 4133
    h, x = ref.make_taps(K), ref.make_input(K, D, n)
    want, bnd = ref.fir(h, x, D, n), ref.bound(h, x, D, n)
    y = ref.fir(mutate(h), mutate(x), D, n)
    frac = float((ref.errors(y, want) > bnd).mean())
    return ref.old_metric(y, want), ref.worst(y, want, bnd), frac


def test_planted_truncation_of_the_filter_operands():
    """Taps and samples TRUNCATED to 16 significand bits (the low eight bits zeroed), float64 sums: 29 times the per-output bound, 90 % of
    the components outside it.  Truncation is biased (every operand shrinks by 1.05e-5 of itself on average), so the largest outputs
    miss the old whole-call metric as well: 2.5e-5 against 1e-5 at 65 taps (3.6e-5 at 9 taps, 2.3e-5 at 129) -- the old metric is not
    asserted to pass here, it is printed.  The unbiased loss of the same bits is the next test."""
    old, new, frac = _planted(ref.truncate_mantissa)
    print("planted operands truncated to 16 bits, 65 taps: old metric %.3g (limit %.0e), worst error / bound %.2f, %.1f %% of the "
          "components outside" % (old, OLD_TOL, new, 100 * frac))
    assert new > 1.0


def test_planted_rounding_of_the_filter_operands():
    """Taps and samples ROUNDED to 16 significand bits, float64 sums: passes the old metric (9.0e-6 of 1e-5), fails the per-output bound
    (10.8 times it, 72 % of the components outside)."""
    def mutate(a):
        a = np.asarray(a)
        if np.iscomplexobj(a):
            return (ref.round_mantissa(a.real) + 1j * ref.round_mantissa(a.imag)).astype(np.complex64)
        return ref.round_mantissa(a).astype(np.float32)

    old, new, frac = _planted(mutate)
    print("planted operands rounded to 16 bits, 65 taps: old metric %.3g (limit %.0e), worst error / bound %.2f, %.1f %% of the "
          "components outside" % (old, OLD_TOL, new, 100 * frac))
    assert old <= OLD_TOL
    assert new > 1.0


# ------------------------------------------------------------------------------------------------------------------------- channelizer

PFB_CPU = ((8, 8, 5), (64, 64, 8), (64, 32, 8), (12, 4, 5), (3, 2, 7), (100, 100, 5))


@pytest.mark.parametrize("M,R,P", PFB_CPU)
def test_channelizer_formula_against_the_oracle(oracle, M, R, P):
    h = pfb_ref.make_taps(M, P)
    steps = 24
    x = pfb_ref.make_input(h.size, R, steps)
    for cm in pfb_ref.maps(M):
        want, bnd = pfb_ref.channelize(h, M, R, cm, x, steps)
        o64 = oracle.pfb(h, steps * R, M, R, cm, x, f64=True)      # (float64 sums, rounded to complex64 on the way out)
        assert np.abs(o64 - want).max() <= 2 * 2.0 ** -24 * np.abs(want).max()
        if M * P <= 400:
            lit = pfb_ref.channelize_literal(h, M, R, cm, x, steps)
            assert np.abs(lit - want).max() <= 1e-12 * np.abs(want).max()
        o32 = oracle.pfb(h, steps * R, M, R, cm, x, f64=False)     # the reference's float32 arithmetic
        r = pfb_ref.worst(o32, want, bnd, len(cm))
        print("channelizer %d / %d, %d taps per arm, %d mapped: float32 oracle worst error / bound %.3f" % (M, R, P, len(cm), r))
        assert r <= 1.0


def test_planted_rounding_of_the_channelizer_twiddles():
    """the M-point DFT with twiddles rounded to 16 significand bits: passes the old metric, fails the per-step bound"""
    M, R, P, steps = 64, 64, 8, 96
    h = pfb_ref.make_taps(M, P)
    x = pfb_ref.make_input(h.size, R, steps)
    cm = list(range(M))
    want, bnd = pfb_ref.channelize(h, M, R, cm, x, steps)
    y = pfb_ref.with_rounded_twiddles(h, M, R, cm, x, steps)
    old, new = pfb_ref.old_metric(y, want), pfb_ref.worst(y, want, bnd, M)
    print("planted 16-bit twiddles, %d channels: old metric %.3g (limit %.0e), worst error / bound %.2f" % (M, old, OLD_TOL, new))
    assert old <= OLD_TOL
    assert new > 1.0
