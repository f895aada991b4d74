"""clBeamformer's C++ block layer: the unit compiles alone, the make() signature is what clenabled.h declares, and the block's
bookkeeping (io signature, item sizes, decimation in POWER mode, what work() hands the library, set_weights size checks) runs on the CPU
over a stub of the C ABI under AddressSanitizer and UBSan (tests/beamform_host_main.cc): a program of its own, nothing loaded into
python.  The pybind class and the CLI row run on the GPU in tests/test_beamform_gpu.py."""
import host_layer


def test_unit_compiles_alone():
    host_layer.unit_compiles_alone("clBeamformer")


def test_make_signature(tmp_path):
    host_layer.probe_compiles(tmp_path,
                              "#include <clenabled/clenabled.h>\n"
                              "using namespace gr::clenabled;\n"
                              "clBeamformer::sptr (*f)(int, int, int, int, int, int, int, int, int, int, bool, const std::vector<int8_t> &, int) = "
                              "&clBeamformer::make;\n"
                              "clBeamformer::sptr nine() { return clBeamformer::make(1, 2, 0, 0, 0, 2, 64, 1024, 64); }\n"
                              "std::string probe(clBeamformer &p) { p.set_weights(p.weights()); p.set_beam_weights(0, std::vector<int8_t>()); p.set_generic(false);\n"
                              "  gr::sync_decimator &d = p; return p.route() + std::to_string(p.num_beams() + p.frame_bytes() + p.out_bytes_per_unit() + d.decimation()); }\n"
                              "int main() { return 0; }\n")


def test_block_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    host_layer.runs_under_sanitizers(tmp_path, "beamform", ["clBeamformer"])
