"""clSpectralSearch's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signatures with the optional spectrum output, item sizes, what work() hands the library item by item, the set_stats
size check, a refused update keeping the old values, every make()-time refusal before the device is looked for) runs on the CPU over a
stub of the C ABI under AddressSanitizer and UBSan (tests/ssearch_host_main.cc): a program of its own, nothing loaded into python.  The
library's own argument checks, plan and helper run without a device in tests/test_ssearch.py; the kernels run on the GPU in
tests/test_ssearch_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clSpectralSearch")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clSpectralSearch::sptr (*f)(int, int, int, int, int, int, int, int, int, const std::vector<float> &, int) =\n"
                              "    &clSpectralSearch::make;\n"
                              "clSpectralSearch::sptr eight() { return clSpectralSearch::make(1, 2, 0, 0, 1024, 1 << 20, 5, 1024); }\n"
                              "std::string probe(clSpectralSearch &p) { p.set_stats(p.inv_sigma()); p.set_generic(false);\n"
                              "  gr::sync_block &b = p;\n"
                              "  return p.route() + std::to_string(p.segment_len() + p.num_bins() + p.records_per_series() + b.history() + p.freq(2, 1280, 1e-3)); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "ssearch", ["clSpectralSearch"])
