"""clFilterbankCleaner's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature with the two optional flag streams, item sizes, output multiple, what work() hands the library, the per-item
copies of the channel flags, set_mask size checks, a refused update keeping the old values) runs on the CPU over a stub of the C ABI
under AddressSanitizer and UBSan (tests/fbclean_host_main.cc): a program of its own, nothing loaded into python.  The pybind class and
the CLI row run on the GPU in tests/test_fbclean_gpu.py."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "gr-clenabled_amd", "host")
INCLUDE = os.path.join(HOST, "include")
UNIT = os.path.join(HOST, "lib", "clFilterbankCleaner_impl.cc")


def test_unit_compiles_alone():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), UNIT],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr


def test_make_signature(tmp_path):
    src = tmp_path / "probe.cc"
    src.write_text("#include <clenabled/clenabled.h>\n"
                   "using namespace gr::clenabled;\n"
                   "clFilterbankCleaner::sptr (*f)(int, int, int, int, int, int, int, double, double, double, double, bool, const std::vector<uint8_t> &, "
                   "int) = &clFilterbankCleaner::make;\n"
                   "clFilterbankCleaner::sptr seven() { return clFilterbankCleaner::make(1, 2, 0, 0, 64, 1024, 256); }\n"
                   "std::string probe(clFilterbankCleaner &p) { p.set_mask(p.mask()); p.set_generic(false); const std::vector<double> l = p.limits();\n"
                   "  p.set_limits(l[0], l[1], l[2], l[3], l[4] != 0); gr::sync_block &b = p;\n"
                   "  return p.route() + std::to_string(p.block_len() + b.history() + b.output_multiple()); }\n"
                   "int main() { return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only", "-I", INCLUDE,
                        "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    exe = tmp_path / "fbclean_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", INCLUDE, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "fbclean_host_main.cc"), UNIT,
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fbclean host ok" in r.stdout, r.stdout + r.stderr
