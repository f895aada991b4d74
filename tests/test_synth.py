"""CPU: clPolyphaseSynthesizer's bookkeeping (mi355_synth_plan needs no device), its argument validation, the soundness of the
yardstick (tests/synth_ref.py: the polyphase form against the closed form) and the convention that ties the block to
clPolyphaseChannelizer: analysis with ones(M), synthesis with [0, 1/M, ...] is a delay of one sample."""
import ctypes as C

import numpy as np
import pytest

import synth_ref as ref

INVALID, UNSUPPORTED = -1, -3


def _plan(L_, K, M, nmap, nframes):
    T = C.c_int(-1)
    nin, nout = C.c_longlong(-1), C.c_longlong(-1)
    rc = L_.mi355_synth_plan(K, M, nmap, nframes, C.byref(T), C.byref(nin), C.byref(nout))
    return rc, (T.value, nin.value, nout.value)


@pytest.mark.parametrize("case", [(6, 23, "half"), (4, 9, "perm"), (5, 5, "half"), (8, 19, "one"), (3, 7, "ident"), (1, 4, "ident")],
                         ids=ref.case_id)
def test_the_two_forms_agree(case):
    M, K, kind = case
    m = ref.make_map(M, kind)
    g = ref.make_taps(K)
    for nframes in (1, 5):
        x = ref.make_input(K, M, ref.nmap_of(M, m), nframes)
        y, z = ref.synth(g, M, m, x, nframes), ref.synth_direct(g, M, m, x, nframes)
        assert y.size == nframes * M
        assert float(np.abs(y - z).max()) < 1e-12 * float(np.abs(z).max())


@pytest.mark.parametrize("M", [2, 3, 4, 8, 12])
def test_round_trip_with_the_channelizer_is_a_delay_of_one(oracle, M):
    """h = ones(M) (K = M, critically sampled, identity map) takes the stream apart, g = [0, 1/M, ..., 1/M] (K = M + 1, T = 2, one
    zero frame of history) puts it together: y[0] = 0, y[n] = x_hist[n - 1].  The oracle rounds its float64 result to complex64, so
    the agreement is float32's, 2^-23 per value."""
    nsteps = 9
    rng = np.random.default_rng(M)
    x_hist = (rng.standard_normal(nsteps * M) + 1j * rng.standard_normal(nsteps * M)).astype(np.complex64)
    u = oracle.pfb(np.ones(M, np.float32), nsteps * M, M, M, np.arange(M, dtype=np.int32), x_hist, f64=True)
    g = np.concatenate([[0.0], np.full(M, 1.0 / M)])
    y = ref.synth(g, M, None, np.concatenate([np.zeros(M, np.complex64), u]), nsteps)
    assert y[0] == 0
    assert float(np.abs(y[1:] - x_hist[:-1]).max()) <= 4 * 2.0 ** -23 * float(np.abs(x_hist).max())


def test_plan_equals_the_yardstick(pkg):
    L_ = pkg.lib()
    for M in (1, 2, 3, 7, 8, 12, 64, 100, 4095, 4096):
        for K in sorted({1, M - 1, M, M + 1, 3 * M - (M // 2 + 1), 3 * M, 8 * M + 5} - {0, -1}):
            for nmap in sorted({1, max(1, M // 2), M}):
                for nframes in (0, 1, 2, 17, 1000):
                    rc, got = _plan(L_, K, M, nmap, nframes)
                    assert rc == 0 and got == ref.plan(K, M, nmap, nframes), (M, K, nmap, nframes, got)
    # 64-bit item counts
    rc, got = _plan(L_, 33, 4, 3, 1 << 40)
    assert rc == 0 and got == ref.plan(33, 4, 3, 1 << 40) and got[2] == 1 << 42
    assert L_.mi355_synth_plan(33, 4, 3, 10, None, None, None) == 0  # NULL outputs are allowed


def test_validation(pkg):
    L_ = pkg.lib()
    for K, M, nmap, nframes in ((5, 0, 1, 1), (5, -3, 1, 1), (0, 4, 4, 1), (-1, 4, 4, 1),     # M or K < 1
                                (5, 4, 0, 1), (5, 4, 5, 1), (5, 4, -1, 1), (5, 4, 4, -1)):    # nmap outside 1 .. M; nframes < 0
        assert _plan(L_, K, M, nmap, nframes)[0] == INVALID, (K, M, nmap, nframes)
    assert _plan(L_, 5, 4096, 4096, 1)[0] == 0
    assert _plan(L_, 5, 4097, 4097, 1)[0] == UNSUPPORTED and b"4097 channels" in L_.mi355_last_error()
    # the table: T M entries, 1048576 at the most, padding counted
    assert _plan(L_, 1048576, 1, 1, 1)[0] == 0
    assert _plan(L_, 1048577, 1, 1, 1)[0] == UNSUPPORTED and b"table entries" in L_.mi355_last_error()
    assert _plan(L_, 256 * 4096, 4096, 1, 1)[0] == 0
    assert _plan(L_, 256 * 4096 + 1, 4096, 1, 1)[0] == UNSUPPORTED
    assert _plan(L_, 262 * 4000 + 1, 4000, 1, 1)[0] == UNSUPPORTED  # 263 x 4000 > 1048576 although K is below it
    # create refuses what it can tell without a device before it looks at the context
    h = C.c_void_p()
    taps = np.ones(9, np.float32)
    tp = taps.ctypes.data_as(C.c_void_p)

    def create(K, M, ch_map, nmap=None, t=tp):
        m = None if ch_map is None else np.asarray(ch_map, np.int32)
        return L_.mi355_synth_create(None, t, K, M, None if m is None else m.ctypes.data_as(C.c_void_p),
                                     (M if m is None else m.size) if nmap is None else nmap, C.byref(h))

    for args in ((9, 0, None, 1), (0, 4, None), (9, 4, None, 0), (9, 4, None, 5)):
        assert create(*args) == INVALID and not h.value, args
    assert create(9, 4, [0, 1, 1]) == INVALID and b"distinct" in L_.mi355_last_error()       # a duplicate
    assert create(9, 4, [0, 4]) == INVALID and create(9, 4, [-1]) == INVALID                  # outside [0, M)
    assert create(9, 4, None, t=None) == INVALID
    assert create(9, 4097, None) == UNSUPPORTED                                               # above the range: its own code
    assert create(9, 4, [2, 0, 3]) == INVALID and b"NULL argument" in L_.mi355_last_error()   # all fine but the context
    assert not h.value
    assert L_.mi355_synth_destroy(None) == 0
    for fn in ("ntaps", "taps_per_arm", "num_channels", "nmap"):
        assert getattr(L_, "mi355_synth_" + fn)(None) == INVALID
    assert L_.mi355_synth_route(None) == b""
    assert L_.mi355_synth_work(None, 1, None, None) == INVALID and L_.mi355_synth_work_dev(None, 1, None, None, None) == INVALID
    assert L_.mi355_synth_set_taps(None, tp, 9) == INVALID


def test_python_class_is_exported(pkg):
    assert pkg.clenabled.clPolyphaseSynthesizer is pkg.clPolyphaseSynthesizer
    for name in ("history", "taps", "set_taps", "taps_per_arm", "route", "plan", "general_work", "work_device"):
        assert callable(getattr(pkg.clPolyphaseSynthesizer, name))
