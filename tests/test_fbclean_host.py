"""clFilterbankCleaner's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature with the two optional flag streams, item sizes, output multiple, what work() hands the library, the per-item
copies of the channel flags, set_mask size checks, a refused update keeping the old values) runs on the CPU over a stub of the C ABI
under AddressSanitizer and UBSan (tests/fbclean_host_main.cc): a program of its own, nothing loaded into python.  The pybind class and
the CLI row run on the GPU in tests/test_fbclean_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clFilterbankCleaner")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clFilterbankCleaner::sptr (*f)(int, int, int, int, int, int, int, double, double, double, double, bool, const std::vector<uint8_t> &, "
                              "int) = &clFilterbankCleaner::make;\n"
                              "clFilterbankCleaner::sptr seven() { return clFilterbankCleaner::make(1, 2, 0, 0, 64, 1024, 256); }\n"
                              "std::string probe(clFilterbankCleaner &p) { p.set_mask(p.mask()); p.set_generic(false); const std::vector<double> l = p.limits();\n"
                              "  p.set_limits(l[0], l[1], l[2], l[3], l[4] != 0); gr::sync_block &b = p;\n"
                              "  return p.route() + std::to_string(p.block_len() + b.history() + b.output_multiple()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "fbclean", ["clFilterbankCleaner"])
