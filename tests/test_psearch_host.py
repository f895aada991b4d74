"""clPulseSearch's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature, item sizes, decimation, history, what work() hands the library, set_stats size checks, a refused update
keeping the old values) runs on the CPU over a stub of the C ABI under AddressSanitizer and UBSan (tests/psearch_host_main.cc): a
program of its own, nothing loaded into python.  The pybind class and the CLI row run on the GPU in tests/test_psearch_gpu.py."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "gr-clenabled_amd", "host")
INCLUDE = os.path.join(HOST, "include")
UNIT = os.path.join(HOST, "lib", "clPulseSearch_impl.cc")


def test_unit_compiles_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), UNIT],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr


def test_make_signature(tmp_path):
    src = tmp_path / "probe.cc"
    src.write_text("#include <clenabled/clenabled.h>\n"
                   "using namespace gr::clenabled;\n"
                   "clPulseSearch::sptr (*f)(int, int, int, int, int, int, int, int, const std::vector<float> &, const std::vector<float> &, int) = "
                   "&clPulseSearch::make;\n"
                   "clPulseSearch::sptr eight() { return clPulseSearch::make(1, 2, 0, 0, 64, 1024, 10, 1024); }\n"
                   "std::string probe(clPulseSearch &p) { p.set_stats(p.mean(), p.inv_sigma()); p.set_generic(false);\n"
                   "  gr::sync_decimator &b = p; return p.route() + std::to_string(p.lookahead() + b.history() + b.decimation()); }\n"
                   "static_assert(sizeof(clPulseSearch::peak) == 8, \"a peak record is 8 bytes\");\n"
                   "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I", INCLUDE,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    exe = tmp_path / "psearch_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "psearch_host_main.cc"), UNIT,
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "psearch host ok" in r.stdout, r.stdout + r.stderr
