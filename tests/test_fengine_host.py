"""clFEngine's device-free entry points and its C++ block layer on the CPU: the unit compiles alone, the make() signature is what
clenabled.h declares, and a program of its own (tests/fengine_host_main.cc) calls mi355_fengine_plan, mi355_fengine_create with a NULL
context, the NULL-handle forms and the argument errors of clFEngine::make under AddressSanitizer and UBSan -- linked against the built
library, nothing loaded into python, no device.  The pybind class and the CLI row run on the GPU in tests/test_fengine_gpu.py."""
import os

import host_layer
from conftest import ROOT

PKG = os.path.join(ROOT, "gr-clenabled_amd")


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clFEngine")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clFEngine::sptr (*f)(int, int, int, int, int, int, int, const std::vector<float> &, int, bool, const std::vector<float> &, int) = "
                              "&clFEngine::make;\n"
                              "clFEngine::sptr seven() { return clFEngine::make(1, 2, 0, 0, 2, 64, 1024); }\n"
                              "std::string probe(clFEngine &p) { p.set_gains(p.gains()); p.set_input_gain(0, std::vector<float>()); p.set_generic(false);\n"
                              "  gr::sync_decimator &d = p; std::vector<uint64_t> c = p.clips(true);\n"
                              "  return p.route() + std::to_string(c.size() + p.frame_bytes() + d.decimation() + d.history()); }\n"
                              "int main() { return 0; }\n")


def test_device_free_entry_points_under_sanitizers(pkg, tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    assert os.path.exists(pkg.LIB_PATH)
    host_layer.runs_under_sanitizers(tmp_path, "fengine", ["clFEngine"],
                                     extra=["-L", PKG, "-lmi355_clenabled", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
