"""clPeriodSearch's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signatures with the optional profile output, item sizes, what work() hands the library item by item, set_stats size
checks, a refused update keeping the old values, every make()-time refusal before the device is looked for) runs on the CPU over a stub
of the C ABI under AddressSanitizer and UBSan (tests/ffa_host_main.cc): a program of its own, nothing loaded into python.  The
library's own argument checks, plan and helpers run without a device in tests/test_ffa.py; the pybind class and the CLI row run on the
GPU in tests/test_ffa_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clPeriodSearch")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clPeriodSearch::sptr (*f)(int, int, int, int, int, int, int, int, int, const std::vector<float> &,\n"
                              "                          const std::vector<float> &, int) = &clPeriodSearch::make;\n"
                              "clPeriodSearch::sptr nine() { return clPeriodSearch::make(1, 2, 0, 0, 64, 250, 251, 12, 7); }\n"
                              "std::string probe(clPeriodSearch &p) { p.set_stats(p.mean(), p.inv_sigma()); p.set_generic(false);\n"
                              "  gr::sync_block &b = p;\n"
                              "  return p.route() + std::to_string(p.segment_len() + p.records_per_series() + b.history() + p.period(250, 0, 1.0)); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "ffa", ["clPeriodSearch"])
