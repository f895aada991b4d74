"""clDedisperser's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature, item sizes, history, what work() hands the library, set_delays size checks, a refused update keeping the old
table) runs on the CPU over a stub of the C ABI under AddressSanitizer and UBSan (tests/dedisp_host_main.cc): a program of its own,
nothing loaded into python.  The pybind class and the CLI row run on the GPU in tests/test_dedisp_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clDedisperser")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clDedisperser::sptr (*f)(int, int, int, int, int, int, int, int, const std::vector<int32_t> &, int) = &clDedisperser::make;\n"
                              "clDedisperser::sptr eight() { return clDedisperser::make(1, 2, 0, 0, 64, 1024, 1024, 1000); }\n"
                              "std::string probe(clDedisperser &p) { p.set_delays(p.delays()); p.set_generic(false);\n"
                              "  gr::sync_block &b = p; return p.route() + std::to_string(p.max_delay() + b.history()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "dedisp", ["clDedisperser"])
