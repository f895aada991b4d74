"""clAccelResampler's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signatures, item sizes, what work() hands the library item by item, the set_trials size check, a refused update
keeping the old table, every make()-time refusal before the device is looked for) runs on the CPU over a stub of the C ABI under
AddressSanitizer and UBSan (tests/accel_host_main.cc): a program of its own, nothing loaded into python.  The library's own argument
checks, plan and helpers run without a device in tests/test_accel.py; the kernels run on the GPU in tests/test_accel_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clAccelResampler")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clAccelResampler::sptr (*f)(int, int, int, int, int, int, const std::vector<long long> &, int) =\n"
                              "    &clAccelResampler::make;\n"
                              "clAccelResampler::sptr seven() { return clAccelResampler::make(1, 2, 0, 0, 64, 1 << 20, {0, 1, -1}); }\n"
                              "std::string probe(clAccelResampler &p) { p.set_trials(p.trials()); p.set_generic(false);\n"
                              "  gr::sync_block &b = p;\n"
                              "  return p.route() + std::to_string(p.segment_len() + p.num_trials() + p.rows() + b.history()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "accel", ["clAccelResampler"])
