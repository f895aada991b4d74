"""clFreqXlatingFIRFilter's C++ block layer: the unit compiles alone, the make() signatures are what clenabled.h declares, and the
block's bookkeeping (io signature, history, the "freq" message port, what work() hands the library, set_taps) runs on the CPU over a
stub of the C ABI under AddressSanitizer and UBSan (tests/xlate_host_main.cc): a program of its own, nothing loaded into python.  The
pybind class and the CLI rows run on the GPU in tests/test_xlate_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clFreqXlatingFIRFilter")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clFreqXlatingFIRFilter::sptr (*f)(int, int, int, int, int, const std::vector<float> &, const std::vector<double> &, double, bool, int) = "
                              "&clFreqXlatingFIRFilter::make;\n"
                              "clFreqXlatingFIRFilter::sptr (*g)(int, int, int, int, int, const std::vector<gr_complex> &, const std::vector<double> &, double, bool, int) = "
                              "&clFreqXlatingFIRFilter::make_ccc;\n"
                              "clFreqXlatingFIRFilter::sptr eight() { return clFreqXlatingFIRFilter::make(1, 2, 0, 0, 16, {1.f, 2.f}, {1e3, -2e3}, 48e3); }\n"
                              "std::string probe(clFreqXlatingFIRFilter &p) { p.set_center_freq(1.0); p.set_center_freq(2.0, 1); p.skip(5); p.set_generic(false);\n"
                              "  p.set_taps(p.taps()); gr::sync_decimator &d = p; return p.route() + std::to_string(p.num_channels() + p.center_freq() + d.decimation()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "xlate", ["clFreqXlatingFIRFilter"])
