"""clPulseSearch's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature, item sizes, decimation, history, what work() hands the library, set_stats size checks, a refused update
keeping the old values) runs on the CPU over a stub of the C ABI under AddressSanitizer and UBSan (tests/psearch_host_main.cc): a
program of its own, nothing loaded into python.  The pybind class and the CLI row run on the GPU in tests/test_psearch_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clPulseSearch")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clPulseSearch::sptr (*f)(int, int, int, int, int, int, int, int, const std::vector<float> &, const std::vector<float> &, int) = "
                              "&clPulseSearch::make;\n"
                              "clPulseSearch::sptr eight() { return clPulseSearch::make(1, 2, 0, 0, 64, 1024, 10, 1024); }\n"
                              "std::string probe(clPulseSearch &p) { p.set_stats(p.mean(), p.inv_sigma()); p.set_generic(false);\n"
                              "  gr::sync_decimator &b = p; return p.route() + std::to_string(p.lookahead() + b.history() + b.decimation()); }\n"
                              "static_assert(sizeof(clPulseSearch::peak) == 8, \"a peak record is 8 bytes\");\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "psearch", ["clPulseSearch"])
