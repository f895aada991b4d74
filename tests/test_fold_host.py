"""clFolder's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's bookkeeping (io
signatures with the optional flag input and hit output, item sizes, decimation, what work() hands the library, the sample counter,
set_models size checks, a refused update keeping the old table, the "models" message port) runs on the CPU over a stub of the C ABI
under AddressSanitizer and UBSan (tests/fold_host_main.cc): a program of its own, nothing loaded into python.  The pybind class and
the CLI row run on the GPU in tests/test_fold_gpu.py."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "gr-clenabled_amd", "host")
INCLUDE = os.path.join(HOST, "include")
UNIT = os.path.join(HOST, "lib", "clFolder_impl.cc")


def test_unit_compiles_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), UNIT],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr


def test_make_signature(tmp_path):
    src = tmp_path / "probe.cc"
    src.write_text("#include <clenabled/clenabled.h>\n"
                   "using namespace gr::clenabled;\n"
                   "clFolder::sptr (*f)(int, int, int, int, int, int, int, int, const std::vector<uint64_t> &, int) = &clFolder::make;\n"
                   "clFolder::sptr nine(const std::vector<uint64_t> &m) { return clFolder::make(1, 2, 0, 0, 64, 1024, 256, 4096, m); }\n"
                   "std::string probe(clFolder &p) { p.set_models(p.models()); p.set_generic(false); p.set_sample(p.sample()); p.skip(0);\n"
                   "  gr::sync_decimator &b = p;\n"
                   "  return p.route() + std::to_string(p.subint_len() + p.nbin() + b.history() + b.decimation()); }\n"
                   "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I", INCLUDE,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    exe = tmp_path / "fold_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fold_host_main.cc"), UNIT,
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fold host ok" in r.stdout, r.stdout + r.stderr
