"""CPU: clSignalSource and clCostasLoop -- the gains and the validation of the C ABI (no device), the float64 restatement
(tests/loops_ref.py) against itself: splitting, stability of every case the GPU tests use, the int cap; and the declarations of
the two C++ blocks (stand-alone and the GNU Radio branch of their units)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import loops_ref as ref

INCLUDE = os.path.join(ROOT, "gr-clenabled_amd", "host", "include")
UNITS = [os.path.join(ROOT, "gr-clenabled_amd", "host", "lib", u) for u in ("clSignalSource_impl.cc", "clCostasLoop_impl.cc")]
INVALID, UNSUPPORTED = -1, -3
COSTAS_TOL = 1e-5


def _plan(pkg, bw, order):
    a, b = C.c_float(-7), C.c_float(-7)
    rc = pkg.lib().mi355_costas_plan(bw, order, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def test_costas_gains_are_the_float32_control_loop_formula(pkg):
    assert _plan(pkg, 0.0628, 2) == (0, 0.16254785656929016, 0.014436298981308937)
    assert ref.costas_gains(0.0628) == (0.16254785656929016, 0.014436298981308937)
    for bw in (0.0, 1e-4, 0.005, 0.0628, 0.1, 0.5, 2.0):
        for order in (2, 4):
            rc, a, b = _plan(pkg, bw, order)
            assert rc == 0 and (a, b) == ref.costas_gains(bw), (bw, order, a, b)


def test_costas_validation(pkg):
    L = pkg.lib()
    for order in (0, 1, 3, 8, -2):
        assert _plan(pkg, 0.0628, order) == (INVALID, 0.0, 0.0)   # the reference's invalid_argument; 8-PSK is commented out there
    assert _plan(pkg, -0.01, 2)[0] == INVALID
    assert _plan(pkg, float("nan"), 4)[0] == INVALID
    assert L.mi355_costas_plan(0.0628, 2, None, None) == 0
    # create: the arguments are judged before the context is touched
    fake_ctx = C.create_string_buffer(4096)
    h = C.c_void_p(1)
    for bw, order, streams, code in [(0.0628, 3, 1, INVALID), (-1.0, 2, 1, INVALID), (0.0628, 2, 0, UNSUPPORTED),
                                     (0.0628, 4, 4097, UNSUPPORTED), (0.0628, 4, -5, UNSUPPORTED)]:
        assert L.mi355_costas_create(fake_ctx, bw, order, streams, C.byref(h)) == code, (bw, order, streams)
        assert not h.value
    assert L.mi355_costas_create(None, 0.0628, 2, 1, C.byref(h)) == INVALID
    assert L.mi355_costas_work_dev(None, 0, None, None, None, None) == INVALID   # no handle is an error even for nothing to do
    assert L.mi355_costas_destroy(None) == 0
    with pytest.raises(ValueError):
        pkg.clCostasLoop(1, 2, 0, 0, 0.0628, 8)   # before any device work, like the reference


def test_sigsource_validation(pkg):
    L = pkg.lib()
    fake_ctx = C.create_string_buffer(4096)
    h = C.c_void_p(1)
    for dtype, rate, wave in [(1, 48000.0, 0), (1, 48000.0, 3), (2, 0.0, 1), (3, -0.0, 2), (4, 48000.0, 1), (0, 48000.0, 1)]:
        assert L.mi355_sigsource_create(fake_ctx, dtype, rate, wave, 1000.0, 1.0, C.byref(h)) == INVALID, (dtype, rate, wave)
        assert not h.value
    assert L.mi355_sigsource_create(None, 1, 48000.0, 1, 1000.0, 1.0, C.byref(h)) == INVALID
    assert L.mi355_sigsource_work_dev(None, 0, None, None) == INVALID
    assert L.mi355_sigsource_destroy(None) == 0


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_wrap_is_the_references_truncating_form():
    assert ref.wrap(1.0) == 1.0 and ref.wrap(ref.TWO_PI) == ref.TWO_PI
    assert abs(ref.wrap(7.0) - (7.0 - ref.TWO_PI)) < 1e-15
    assert abs(ref.wrap(-20.0) - (-20.0 + 3 * ref.TWO_PI)) < 1e-14   # toward zero: the sign is kept
    assert ref.sig_advance(0.0, np.pi / 4, 8192) < 1e-9


@pytest.mark.parametrize("order,streams", [(2, 1), (4, 1), (2, 100), (4, 100)])
def test_splitting_a_stream_in_the_restatement_is_bit_identical(order, streams):
    n = 1000
    x, _ = ref.costas_input(order, streams, n)
    whole = ref.costas(x, order, ref.LOOP_BW, streams)
    outs, freqs, state, at = [], [], None, 0
    for m in (1, 63, 500, n - 564):
        o, f, state = ref.costas(x[at * streams:(at + m) * streams], order, ref.LOOP_BW, streams, state=state)
        outs.append(o); freqs.append(f); at += m
    assert np.array_equal(np.concatenate(outs), whole[0]) and np.array_equal(np.concatenate(freqs), whole[1])
    for a, b in zip(state, whole[2]):
        assert np.array_equal(a, b)
    if streams == 1:  # and the scalar form is the same loop
        o, f, st = ref.costas_scalar(x, order, ref.LOOP_BW)
        assert np.abs(o - whole[0]).max() < 1e-9 and np.abs(f - whole[1]).max() < 1e-9


@pytest.mark.parametrize("order", ref.COSTAS_ORDERS)
@pytest.mark.parametrize("streams", ref.COSTAS_STREAMS)
def test_every_gpu_case_is_stable_under_trig_noise(order, streams):
    """1e-9 relative noise on every sin / cos moves no output of a case by more than a tenth of the tolerance: no input sits near a
    sign flip of the (discontinuous) order-4 detector or near an unstable phase, so a device whose trig differs in the last bits
    is judged by its arithmetic and not by luck."""
    n = max(ref.COSTAS_NITEMS)   # the shorter cases are prefixes of this one
    x, _ = ref.costas_input(order, streams, n)
    clean = ref.costas_expected(order, streams, n)
    noisy = ref.costas(x, order, ref.LOOP_BW, streams, trig_noise=1e-9, rng=np.random.default_rng(5))
    scale = float(np.abs(x).max())
    assert np.abs(noisy[0] - clean[0]).max() <= 0.1 * COSTAS_TOL * scale
    assert np.abs(noisy[1] - clean[1]).max() <= 0.1 * COSTAS_TOL


def test_the_start_state_case_is_stable():
    order, streams, n, start = ref.COSTAS_START
    x, _ = ref.costas_input(order, streams, n)
    clean = ref.costas(x, order, ref.LOOP_BW, streams, state=start)
    noisy = ref.costas(x, order, ref.LOOP_BW, streams, state=start, trig_noise=1e-9, rng=np.random.default_rng(7))
    assert np.abs(noisy[0] - clean[0]).max() <= 0.1 * COSTAS_TOL * float(np.abs(x).max())
    assert np.abs(noisy[1] - clean[1]).max() <= 0.1 * COSTAS_TOL


def test_the_three_piece_case_is_stable():
    order, streams, _ = ref.COSTAS_PIECES
    x, _ = ref.costas_pieces_input()
    clean = ref.costas_pieces_expected()
    noisy = ref.costas(x, order, ref.LOOP_BW, streams, trig_noise=1e-9, rng=np.random.default_rng(8))
    assert np.abs(noisy[0] - clean[0]).max() <= 0.1 * COSTAS_TOL * float(np.abs(x).max())
    assert np.abs(noisy[1] - clean[1]).max() <= 0.1 * COSTAS_TOL


def test_the_long_case_is_stable_and_locks():
    x, off = ref.costas_long_input()
    clean = ref.costas_long_expected()
    noisy = ref.costas_scalar(x, ref.COSTAS_LONG[0], ref.LOOP_BW, trig_noise=1e-9, rng=np.random.default_rng(6))
    assert np.abs(noisy[0] - clean[0]).max() <= 0.1 * COSTAS_TOL * float(np.abs(x).max())
    assert abs(clean[2][1] - off[0]) <= 0.1 * abs(off[0])            # locked: the loop frequency is the offset
    assert abs(off[0]) * ref.COSTAS_LONG[1] > 100 * ref.TWO_PI       # over many wraps of the phase


def test_grid_streams_lock_to_their_offsets():
    """what the loop is for: after 4097 items every stream's frequency is near its offset (the instantaneous value jitters with
    the noise, hence a third)"""
    for order in ref.COSTAS_ORDERS:
        _, off = ref.costas_input(order, 256, 4097)
        freq = ref.costas_expected(order, 256, 4097)[2][1]
        assert np.median(np.abs(freq - off)) < 0.002 and np.all(np.abs(freq - off) < 0.01 + np.abs(off) / 3)


def test_int_cases_stay_off_the_integers():
    """the int output is compared exactly, except within 1e-6 of an integer; at most 0.1 % of the positions of any int case of
    the GPU tests may be such positions"""
    for ratio, amp, wave in ref.SIG_INT_CASES:
        inc = ref.sig_inc(ratio * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
        for n in ref.SIG_N:
            v, _ = ref.sig_call(ref.SIG_INT_PHASE, inc, n, amp, "int", wave)
            assert ref.near_integer(v).sum() <= ref.INT_CAP * n, (ratio, wave, n)
        pos, vs = ref.SIG_INT_PHASE, []
        for n in ref.SIG_RAGGED:
            v, pos = ref.sig_call(pos, inc, n, amp, "int", wave)
            vs.append(v)
        v = np.concatenate(vs)
        assert ref.near_integer(v).sum() <= ref.INT_CAP * len(v)


def test_signal_source_consecutive_calls_are_one_stream():
    """the host-side advance: a run of calls continues the tone (to the rounding of the wrapped phase)"""
    inc = ref.sig_inc(0.01234 * ref.SIG_SAMP_RATE, ref.SIG_SAMP_RATE)
    pos, vs = 0.0, []
    for n in ref.SIG_RAGGED:
        v, pos = ref.sig_call(pos, inc, n, 1.0, "complex", 1)
        vs.append(v)
    total = sum(ref.SIG_RAGGED)
    one = np.exp(1j * inc * np.arange(total))
    assert np.abs(np.concatenate(vs) - one).max() < 1e-9
    assert -ref.TWO_PI <= pos <= ref.TWO_PI


# ---------------------------------------------------------------------------------------------------------- the C++ blocks
def test_make_signatures_compile_against_clenabled_h(tmp_path):
    src = tmp_path / "tu.cc"
    src.write_text("#include <clenabled/clenabled.h>\n"
                   "using namespace gr::clenabled;\n"
                   "clSignalSource::sptr (*f)(int, int, int, int, int, double, int, double, float, int) = &clSignalSource::make;\n"
                   "clCostasLoop::sptr (*g)(int, int, int, int, float, int, int) = &clCostasLoop::make;\n"
                   "float probe(clCostasLoop &c) { c.set_loop_bandwidth(0.1f); c.set_frequency(0.f); c.set_phase(0.f);\n"
                   "  return c.get_loop_bandwidth() + c.get_alpha() + c.get_beta() + c.get_frequency() + c.get_phase(); }\n"
                   "clSignalSource::sptr nine() { return clSignalSource::make(1, 1, 2, 0, 0, 48000.0, 1, 1000.0, 1.0f); }\n"
                   "clCostasLoop::sptr six() { return clCostasLoop::make(1, 2, 0, 0, 0.0628f, 4); }\n"
                   "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I", INCLUDE,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("unit", UNITS, ids=[os.path.basename(u) for u in UNITS])
@pytest.mark.parametrize("gnuradio", [False, True], ids=["standalone", "gnuradio"])
def test_units_compile_alone_and_against_the_api_model(unit, gnuradio):
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "include")]
    if gnuradio:
        cmd += ["-DMI355_WITH_GNURADIO", "-I", os.path.join(ROOT, "tests", "gr_api_mock")]
    r = subprocess.run(cmd + [unit], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr


def test_dropin_module_exports_both_blocks():
    import sys
    code = "import clenabled as c; assert callable(c.clSignalSource) and callable(c.clCostasLoop); print('ok')"
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gr-clenabled_amd", "python"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
