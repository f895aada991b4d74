"""clPowerSpectrum's C++ block layer: the unit compiles alone, the block's bookkeeping (forecast,
history, what general_work() hands the library and consumes) runs on the CPU over a stub of the C ABI under AddressSanitizer and
UBSan (tests/pspec_host_main.cc), and on the GPU the pybind module and the CLI rows are checked against tests/pspec_ref.py."""
import glob
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import host_layer
from conftest import GPU_ARGS, ROOT, relerr
import pspec_ref as ref

CLI = os.path.join(ROOT, "gr-clenabled_amd", "test-clenabled-mi355")


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clPowerSpectrum")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clPowerSpectrum::sptr (*f)(int, int, int, int, int, int, const std::vector<float> &, int, bool, bool, float, int) = &clPowerSpectrum::make;\n"
                              "clPowerSpectrum::sptr six() { return clPowerSpectrum::make(1, 2, 0, 0, 1024, 16); }\n"
                              "std::string probe(clPowerSpectrum &p) { p.set_scale(1.f); p.set_window({}); p.set_generic(false);\n"
                              "  return p.route() + std::to_string(p.fft_size() + p.navg() + p.hop()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "pspec", ["clPowerSpectrum"])


def _pybind():
    mods = glob.glob(os.path.join(ROOT, "gr-clenabled_amd", "clenabled_python*.so"))
    assert mods, "pybind module not built"
    spec = importlib.util.spec_from_file_location("clenabled_python", mods[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,H", [(64, 5, 48), (100, 3, 130)])
def test_pybind_block_over_uneven_pieces(gpu, N, K, H):
    """general_work() as the scheduler calls it: whatever input there is is offered, the block makes the whole spectra that input and
    the output room allow and consumes spectra x navg x hop; the pieces together are one pspec() of the stream."""
    mod = _pybind()
    w = ref.hann(N)
    blk = mod.clPowerSpectrum(*GPU_ARGS, N, K, w.tolist(), H, True, False, 0.5)
    assert (blk.fft_size(), blk.navg(), blk.hop()) == (N, K, H) and blk.history() == max(N - H, 0) + 1
    assert blk.route().startswith("fused pow2" if N == 64 else "generic")
    assert blk.forecast(7) == max(ref.plan(N, K, H, 7)[0], 7 * K * H)
    total = 40
    x = ref.make_input(max(ref.plan(N, K, H, total)[0], total * K * H), seed=N)  # (hop > fft_size: the skipped items are consumed too)
    y = np.full((total + 3) * N, np.nan, np.float32)
    rng = np.random.default_rng(4)
    pos, made = 0, 0
    one = ref.plan(N, K, H, 1)[0]
    for _ in range(2000):
        if made == total:
            break
        avail = min(int(rng.choice([N - 1, one - 1, one, one + K * H - 1, 3 * one, 5000])), x.size - pos)
        room = min(int(rng.choice([0, 1, 2, 9])), y.size // N - made)
        fit = avail // (K * H) if H > N else (((avail - N) // H + 1) // K if avail >= N else 0)  # never more consumed than offered
        want = min(fit, room)
        produced, consumed = blk.general_work(room, [x[pos:pos + avail]], [y[made * N:(made + room) * N]])
        assert (produced, consumed) == (want, want * K * H)
        pos, made = pos + consumed, made + produced
    assert made == total and pos == total * K * H and pos <= x.size
    assert relerr(y[:total * N].reshape(total, N), ref.pspec(x, N, K, H, total, w, True, scale=0.5)) <= ref.TOL
    assert np.all(np.isnan(y[total * N:]))
    blk.set_scale(1.0)
    blk.set_window([])
    blk.set_generic(True)
    assert blk.route().startswith("generic")
    y2 = np.full(2 * N, np.nan, np.float32)
    assert blk.general_work(2, [x], [y2]) == (2, 2 * K * H)
    assert relerr(y2.reshape(2, N), ref.pspec(x, N, K, H, 2, None, True)) <= ref.TOL


@pytest.mark.gpu
def test_cli_pspec_only(gpu):
    r = subprocess.run([CLI, "--pspec-only", "--iterations", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(rows) == 3 and all(l.startswith("clPowerSpectrum") and l.rstrip().endswith("ok") for l in rows), r.stdout
