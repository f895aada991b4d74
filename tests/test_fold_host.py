"""clFolder's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's bookkeeping (io
signatures with the optional flag input and hit output, item sizes, decimation, what work() hands the library, the sample counter,
set_models size checks, a refused update keeping the old table, the "models" message port) runs on the CPU over a stub of the C ABI
under AddressSanitizer and UBSan (tests/fold_host_main.cc): a program of its own, nothing loaded into python.  The pybind class and
the CLI row run on the GPU in tests/test_fold_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clFolder")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clFolder::sptr (*f)(int, int, int, int, int, int, int, int, const std::vector<uint64_t> &, int) = &clFolder::make;\n"
                              "clFolder::sptr nine(const std::vector<uint64_t> &m) { return clFolder::make(1, 2, 0, 0, 64, 1024, 256, 4096, m); }\n"
                              "std::string probe(clFolder &p) { p.set_models(p.models()); p.set_generic(false); p.set_sample(p.sample()); p.skip(0);\n"
                              "  gr::sync_decimator &b = p;\n"
                              "  return p.route() + std::to_string(p.subint_len() + p.nbin() + b.history() + b.decimation()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "fold", ["clFolder"])
