"""clBeamformer's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature, item sizes, decimation in POWER mode, what work() hands the library, set_weights size checks) runs on the CPU
over a stub of the C ABI under AddressSanitizer and UBSan (tests/beamform_host_main.cc): a program of its own, nothing loaded into
python.  The pybind class and the CLI row run on the GPU in tests/test_beamform_gpu.py."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "gr-clenabled_amd", "host")
INCLUDE = os.path.join(HOST, "include")
UNIT = os.path.join(HOST, "lib", "clBeamformer_impl.cc")


def test_unit_compiles_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), UNIT],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr


def test_make_signature(tmp_path):
    src = tmp_path / "probe.cc"
    src.write_text("#include <clenabled/clenabled.h>\n"
                   "using namespace gr::clenabled;\n"
                   "clBeamformer::sptr (*f)(int, int, int, int, int, int, int, int, int, int, bool, const std::vector<int8_t> &, int) = "
                   "&clBeamformer::make;\n"
                   "clBeamformer::sptr nine() { return clBeamformer::make(1, 2, 0, 0, 0, 2, 64, 1024, 64); }\n"
                   "std::string probe(clBeamformer &p) { p.set_weights(p.weights()); p.set_beam_weights(0, std::vector<int8_t>()); p.set_generic(false);\n"
                   "  gr::sync_decimator &d = p; return p.route() + std::to_string(p.num_beams() + p.frame_bytes() + p.out_bytes_per_unit() + d.decimation()); }\n"
                   "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I", INCLUDE,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    exe = tmp_path / "beamform_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "beamform_host_main.cc"), UNIT,
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "beamform host ok" in r.stdout, r.stdout + r.stderr
