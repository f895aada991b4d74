// pybind11 module `clenabled_python`: the gr::clenabled block classes of the MI355X build.
//
// Takes the place of the reference's python/bindings/python_bindings.cc:57-95 + the per-block *_python.cc files: every block is
// constructed through its static make() (py::init(&X::make)), positional order exactly the make() order, so the `make:`
// templates of grc/clenabled_*.block.yml construct the same objects.  Keyword names follow the C++ parameter names of
// clenabled.h -- for clFFT that is the .cc order of the reference (its generated binding carries the header's mislabelled
// names; GRC passes positionally).
// With GNU Radio (MI355_WITH_GNURADIO, set by CMake when find_package(Gnuradio) succeeds) the classes derive from GNU
// Radio's bound gr::sync_block / gr::block / gr::basic_block, i.e. they connect in flowgraphs; without it the same source
// builds a stand-alone module (no flowgraph, work()/general_work() callable on numpy buffers) used by tests/test_pybind.py.
#include <pybind11/complex.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <clenabled/clenabled.h>

#include <string>
#include <type_traits>

namespace py = pybind11;
using namespace gr::clenabled;

#ifdef MI355_WITH_GNURADIO
#define SYNC_BASES , gr::sync_block, gr::block, gr::basic_block
#define DECIM_BASES , gr::sync_decimator, gr::sync_block, gr::block, gr::basic_block
#define BLOCK_BASES , gr::block, gr::basic_block
#else
#define SYNC_BASES
#define DECIM_BASES
#define BLOCK_BASES
#endif

namespace {
// numpy buffers -> the pointer vectors work() takes (stand-alone use and tests; inside GNU Radio the scheduler calls work()).
// The scheduler guarantees buffer sizes; a Python caller does not, so every buffer is checked against the block's own io
// signature, history and decimation before a pointer reaches work(): C-contiguous, and at least as many bytes as the call reads
// or writes.
void need(bool ok, const std::string &what)
{
    if (!ok) throw py::value_error(what);
}
template <class B> size_t item_size(const B &b, bool input, size_t k)
{
    auto sig = input ? b.input_signature() : b.output_signature();
    return (size_t)sig->sizeof_stream_item((int)k);
}
gr_vector_const_void_star in_ptrs(const std::vector<py::array> &a)
{
    gr_vector_const_void_star v;
    for (auto &x : a) {
        need((x.flags() & py::array::c_style) != 0, "input buffers must be C-contiguous numpy arrays");
        v.push_back(x.data());
    }
    return v;
}
gr_vector_void_star out_ptrs(std::vector<py::array> &a)
{
    gr_vector_void_star v;
    for (auto &x : a) {
        need((x.flags() & py::array::c_style) != 0 && x.writeable(), "output buffers must be writable C-contiguous numpy arrays");
        v.push_back(x.mutable_data());
    }
    return v;
}
template <class B> unsigned decimation_of(const B &b)
{
    if constexpr (std::is_base_of<gr::sync_decimator, B>::value) return b.decimation();
    else return 1;
}
template <class B> int call_work(B &b, int noutput_items, const std::vector<py::array> &in, std::vector<py::array> out)
{
    need(noutput_items >= 0, "noutput_items is negative");
    auto i = in_ptrs(in);
    auto o = out_ptrs(out);
    const size_t items_in = (size_t)noutput_items * decimation_of(b) + (b.history() > 0 ? b.history() - 1 : 0);
    for (size_t k = 0; k < in.size(); k++)
        need((size_t)in[k].nbytes() >= items_in * item_size(b, true, k),
             "input " + std::to_string(k) + " holds fewer than noutput_items * decimation + history - 1 items");
    for (size_t k = 0; k < out.size(); k++)
        need((size_t)out[k].nbytes() >= (size_t)noutput_items * item_size(b, false, k),
             "output " + std::to_string(k) + " holds fewer than noutput_items items");
    return b.work(noutput_items, i, o);
}
template <class B> int call_general_work(B &b, int noutput_items, const std::vector<py::array> &in, std::vector<py::array> out)
{
    need(noutput_items >= 0, "noutput_items is negative");
    auto i = in_ptrs(in);
    auto o = out_ptrs(out);
    gr_vector_int n(in.size(), 0), req(in.size(), 0);
    for (size_t k = 0; k < in.size(); k++) {  // items, not array elements: one item = sizeof_stream_item bytes
        const size_t isz = item_size(b, true, k);
        n[k] = isz ? (int)((size_t)in[k].nbytes() / isz) : 0;
    }
    b.forecast(noutput_items, req);
    for (size_t k = 0; k < in.size(); k++)
        need(n[k] >= req[k], "input " + std::to_string(k) + " holds fewer items than forecast() asks for");
    for (size_t k = 0; k < out.size(); k++)
        need((size_t)out[k].nbytes() >= (size_t)noutput_items * item_size(b, false, k),
             "output " + std::to_string(k) + " holds fewer than noutput_items items");
    return b.general_work(noutput_items, n, i, o);
}
}  // namespace

PYBIND11_MODULE(clenabled_python, m)
{
    m.doc() = "gr-clenabled blocks, MI355X build (HIP kernels behind the reference's block API)";
#ifdef MI355_WITH_GNURADIO
    py::module::import("gnuradio.gr");  // the base classes' bindings
    m.attr("with_gnuradio") = true;
#else
    m.attr("with_gnuradio") = false;
#endif
    // include/clenabled/GRCLBase.h:57-70, clMathOpTypes.h:11-20, clFFT.h:28-29
    m.attr("DTYPE_COMPLEX") = DTYPE_COMPLEX; m.attr("DTYPE_FLOAT") = DTYPE_FLOAT; m.attr("DTYPE_INT") = DTYPE_INT;
    m.attr("DTYPE_SHORT") = DTYPE_SHORT; m.attr("DTYPE_BYTE") = DTYPE_BYTE; m.attr("DTYPE_PACKEDXY") = DTYPE_PACKEDXY;
    m.attr("OCLTYPE_GPU") = OCLTYPE_GPU; m.attr("OCLTYPE_ACCELERATOR") = OCLTYPE_ACCELERATOR; m.attr("OCLTYPE_CPU") = OCLTYPE_CPU;
    m.attr("OCLTYPE_ANY") = OCLTYPE_ANY; m.attr("OCLDEVICESELECTOR_FIRST") = OCLDEVICESELECTOR_FIRST;
    m.attr("OCLDEVICESELECTOR_SPECIFIC") = OCLDEVICESELECTOR_SPECIFIC;
    m.attr("MATHOP_MULTIPLY") = MATHOP_MULTIPLY; m.attr("MATHOP_ADD") = MATHOP_ADD; m.attr("MATHOP_SUBTRACT") = MATHOP_SUBTRACT;
    m.attr("MATHOP_COMPLEX_CONJUGATE") = MATHOP_COMPLEX_CONJUGATE; m.attr("MATHOP_MULTIPLY_CONJUGATE") = MATHOP_MULTIPLY_CONJUGATE;
    m.attr("CLFFT_FORWARD") = CLFFT_FORWARD; m.attr("CLFFT_BACKWARD") = CLFFT_BACKWARD;
    m.attr("CLXCORR_TRIANGULAR_ORDER") = CLXCORR_TRIANGULAR_ORDER; m.attr("CLXCORR_FULL_MATRIX") = CLXCORR_FULL_MATRIX;

    py::class_<clMathOp SYNC_BASES, std::shared_ptr<clMathOp>>(m, "clMathOp")
        .def(py::init(&clMathOp::make), py::arg("idataType"), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"),
             py::arg("devId"), py::arg("operatorType"), py::arg("setDebug") = 0)
        .def("work", &call_work<clMathOp>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clMathConst SYNC_BASES, std::shared_ptr<clMathConst>>(m, "clMathConst")
        .def(py::init(&clMathConst::make), py::arg("idataType"), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"),
             py::arg("devId"), py::arg("fValue"), py::arg("operatorType"), py::arg("setDebug") = 0)
        .def("k", &clMathConst::k)          // GRC callback set_k(${const}); also what the reference exposes on ControlPort
        .def("set_k", &clMathConst::set_k, py::arg("newValue"))
        .def("work", &call_work<clMathConst>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clFFT SYNC_BASES, std::shared_ptr<clFFT>>(m, "clFFT")
        .def(py::init(&clFFT::make), py::arg("fftSize"), py::arg("clFFTDir"), py::arg("window"), py::arg("idataType"),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("setDebug") = 0,
             py::arg("num_streams") = 1, py::arg("shift") = false)
        .def("work", &call_work<clFFT>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clFilter DECIM_BASES, std::shared_ptr<clFilter>>(m, "clFilter")
        .def(py::init(&clFilter::make), py::arg("openclPlatform"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("decimation"), py::arg("taps"), py::arg("nthreads") = 1, py::arg("setDebug") = 0, py::arg("use_time") = DEFAULT_USE_TIME_DOMAIN_SETTING)
        .def("set_taps2", &clFilter::set_taps2, py::arg("taps"))
        .def("taps", &clFilter::taps)
        .def("set_nthreads", &clFilter::set_nthreads, py::arg("n"))
        .def("work", &call_work<clFilter>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clComplexFilter DECIM_BASES, std::shared_ptr<clComplexFilter>>(m, "clComplexFilter")
        .def(py::init(&clComplexFilter::make), py::arg("openclPlatform"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("decimation"), py::arg("taps"), py::arg("nthreads") = 1, py::arg("setDebug") = 0)
        .def("set_taps2", &clComplexFilter::set_taps2, py::arg("taps"))
        .def("taps", &clComplexFilter::taps)
        .def("work", &call_work<clComplexFilter>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clPolyphaseChannelizer BLOCK_BASES, std::shared_ptr<clPolyphaseChannelizer>>(m, "clPolyphaseChannelizer")
        .def(py::init(&clPolyphaseChannelizer::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"),
             py::arg("devId"), py::arg("taps"), py::arg("buf_items"), py::arg("num_channels"), py::arg("ninputs_per_iter"), py::arg("ch_map"),
             py::arg("setDebug") = 0)
        .def("general_work", &call_general_work<clPolyphaseChannelizer>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clXEngine BLOCK_BASES, std::shared_ptr<clXEngine>>(m, "clXEngine")
        .def(py::init(&clXEngine::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("setDebug"), py::arg("data_type"), py::arg("polarization"), py::arg("num_inputs"), py::arg("output_format"),
             py::arg("first_channel"), py::arg("num_channels"), py::arg("integration"), py::arg("antenna_list"), py::arg("output_file") = false,
             py::arg("file_base") = "", py::arg("rollover_size_mb") = 0, py::arg("internal_synchronizer") = false, py::arg("sync_timestamp") = 0,
             py::arg("object_name") = "", py::arg("starting_chan_center_freq") = 0.0, py::arg("channel_width") = 0.0,
             py::arg("disable_output") = false, py::arg("pipeline_integration") = 0)
        .def("get_input_buffer_size", &clXEngine::get_input_buffer_size)
        .def("get_output_buffer_size", &clXEngine::get_output_buffer_size)
        .def("integrations_delivered", &clXEngine::integrations_delivered)
        .def("set_shard_devices", &clXEngine::set_shard_devices, py::arg("device_ids"), py::arg("windows_per_exchange") = 4)  // not in the reference: several devices behind one block
        .def("shard_devices", &clXEngine::shard_devices)
        .def("synchronized", &clXEngine::synchronized)
        .def("general_work", &call_general_work<clXEngine>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"))
        .def("stop", [](clXEngine &x) { return x.stop(); });  // (a member of the virtual base: no pointer-to-member through it)

    // ---- the remaining elementwise family and the reference correlator: python/bindings/clLog_python.cc etc.
#define MI355_BIND_ELEM(NAME, ...)                                                                                     \
    py::class_<NAME SYNC_BASES, std::shared_ptr<NAME>>(m, #NAME)                                                       \
        .def(py::init(&NAME::make), __VA_ARGS__)                                                                       \
        .def("work", &call_work<NAME>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"))
#define MI355_DEV_ARGS py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId")
    MI355_BIND_ELEM(clLog, MI355_DEV_ARGS, py::arg("nValue"), py::arg("kValue"), py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clSNR, MI355_DEV_ARGS, py::arg("nValue"), py::arg("kValue"), py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clComplexToMag, MI355_DEV_ARGS, py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clComplexToArg, MI355_DEV_ARGS, py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clComplexToMagPhase, MI355_DEV_ARGS, py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clMagPhaseToComplex, MI355_DEV_ARGS, py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clQuadratureDemod, py::arg("gain"), MI355_DEV_ARGS, py::arg("setDebug") = 0);
    MI355_BIND_ELEM(clxcorrelate_fft_vcf, py::arg("fftSize"), py::arg("num_inputs"), MI355_DEV_ARGS, py::arg("input_type") = 1);
#undef MI355_DEV_ARGS
#undef MI355_BIND_ELEM

    // time-domain lag search (lib/clXCorrelate_impl.cc): no outputs; work() takes the input buffers only
    py::class_<clXCorrelate SYNC_BASES, std::shared_ptr<clXCorrelate>>(m, "clXCorrelate")
        .def(py::init(&clXCorrelate::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("setDebug"), py::arg("num_inputs"), py::arg("signal_length"), py::arg("data_type"), py::arg("data_size"),
             py::arg("max_search_index"), py::arg("decim_frames"), py::arg("async_") = false)
        .def("work",
             [](clXCorrelate &b, int noutput_items, const std::vector<py::array> &in) {
                 need(noutput_items >= 0, "noutput_items is negative");
                 auto i = in_ptrs(in);
                 const size_t items = (size_t)std::min(noutput_items, b.signal_length());
                 for (size_t k = 0; k < in.size(); k++)
                     need((size_t)in[k].nbytes() >= items * item_size(b, true, k), "input " + std::to_string(k) + " holds fewer than a frame");
                 gr_vector_void_star o;
                 return b.work(noutput_items, i, o);
             },
             py::arg("noutput_items"), py::arg("input_items"))
        .def("max_shift", &clXCorrelate::max_shift)
        .def("wait", &clXCorrelate::wait)
#ifndef MI355_WITH_GNURADIO
        // the published PDUs of the stand-alone build, oldest first: [(corrvect, corrective_lags), ...]
        .def("pop_pdus", [](clXCorrelate &b) {
            py::list out;
            gr::shim_message msg;
            while (b.pop_message(msg)) out.append(py::make_tuple(msg.f32, msg.s32));
            return out;
        })
#endif
        ;

    // NCO and carrier recovery (lib/clSignalSource_impl.cc, lib/clCostasLoop_impl.cc); work() of the source takes no inputs
    py::class_<clSignalSource SYNC_BASES, std::shared_ptr<clSignalSource>>(m, "clSignalSource")
        .def(py::init(&clSignalSource::make), py::arg("idataType"), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"),
             py::arg("devId"), py::arg("samp_rate"), py::arg("waveform"), py::arg("freq"), py::arg("amplitude"), py::arg("setDebug") = 0)
        .def("set_frequency", &clSignalSource::set_frequency, py::arg("frequency"))
        .def("set_phase", &clSignalSource::set_phase, py::arg("angle_pos"))
        .def("get_angle_pos", &clSignalSource::get_angle_pos)
        .def("get_angle_rate", &clSignalSource::get_angle_rate)
        .def("work", &call_work<clSignalSource>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    py::class_<clCostasLoop SYNC_BASES, std::shared_ptr<clCostasLoop>>(m, "clCostasLoop")
        .def(py::init(&clCostasLoop::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("loop_bw"), py::arg("order"), py::arg("setDebug") = 0)
        .def("set_loop_bandwidth", &clCostasLoop::set_loop_bandwidth, py::arg("bw"))
        .def("get_loop_bandwidth", &clCostasLoop::get_loop_bandwidth)
        .def("get_alpha", &clCostasLoop::get_alpha)
        .def("get_beta", &clCostasLoop::get_beta)
        .def("get_frequency", &clCostasLoop::get_frequency)
        .def("get_phase", &clCostasLoop::get_phase)
        .def("set_frequency", &clCostasLoop::set_frequency, py::arg("freq"))
        .def("set_phase", &clCostasLoop::set_phase, py::arg("phase"))
        .def("work", &call_work<clCostasLoop>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // polyphase interpolating / rational-rate FIR (lib/clRationalResampler_impl.cc).  Complex taps construct the _ccc form.  general_work()
    // is offered whatever the input array holds (history included) and returns (produced, consumed): the block decides how many
    // outputs that input allows, as under the scheduler.
    py::class_<clRationalResampler BLOCK_BASES, std::shared_ptr<clRationalResampler>>(m, "clRationalResampler")
        .def(py::init(&clRationalResampler::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("interpolation"), py::arg("decimation"), py::arg("taps"), py::arg("setDebug") = 0)
        .def_static("make_ccc", &clRationalResampler::make_ccc, py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"),
                    py::arg("devId"), py::arg("interpolation"), py::arg("decimation"), py::arg("taps"), py::arg("setDebug") = 0)
        .def("taps", &clRationalResampler::taps)
        .def("set_taps", &clRationalResampler::set_taps, py::arg("taps"))
        .def("interpolation", &clRationalResampler::interpolation)
        .def("decimation", &clRationalResampler::decimation)
        .def("history", [](clRationalResampler &b) { return b.history(); })
        .def("forecast",
             [](clRationalResampler &b, int noutput_items) {
                 gr_vector_int req(1, 0);
                 b.forecast(noutput_items, req);
                 return req[0];
             },
             py::arg("noutput_items"))
#ifndef MI355_WITH_GNURADIO
        // stand-alone build only: consume_each() outside a flowgraph has nothing to report to
        .def("general_work",
             [](clRationalResampler &b, int noutput_items, const std::vector<py::array> &in, std::vector<py::array> out) {
                 need(noutput_items >= 0, "noutput_items is negative");
                 need(in.size() == 1 && out.size() == 1, "one input and one output");
                 auto i = in_ptrs(in);
                 auto o = out_ptrs(out);
                 gr_vector_int n(1, (int)((size_t)in[0].nbytes() / sizeof(gr_complex)));
                 need((size_t)out[0].nbytes() >= (size_t)noutput_items * sizeof(gr_complex), "output 0 holds fewer than noutput_items items");
                 const long before = b.nitems_consumed(0);
                 const int produced = b.general_work(noutput_items, n, i, o);
                 return py::make_tuple(produced, b.nitems_consumed(0) - before);
             },
             py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"))
#endif
        ;

    // polyphase synthesis bank (lib/clPolyphaseSynthesizer_impl.cc).  general_work() is offered whatever the input array holds (history
    // included) and returns (produced, consumed): whole frames only, as under the scheduler.
    py::class_<clPolyphaseSynthesizer BLOCK_BASES, std::shared_ptr<clPolyphaseSynthesizer>>(m, "clPolyphaseSynthesizer")
        .def(py::init(&clPolyphaseSynthesizer::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("taps"), py::arg("num_channels"), py::arg("ch_map") = std::vector<int>(), py::arg("setDebug") = 0)
        .def("taps", &clPolyphaseSynthesizer::taps)
        .def("set_taps", &clPolyphaseSynthesizer::set_taps, py::arg("taps"))
        .def("taps_per_arm", &clPolyphaseSynthesizer::taps_per_arm)
        .def("num_channels", &clPolyphaseSynthesizer::num_channels)
        .def("nmap", &clPolyphaseSynthesizer::nmap)
        .def("route", &clPolyphaseSynthesizer::route)
        .def("history", [](clPolyphaseSynthesizer &b) { return b.history(); })
        .def("forecast",
             [](clPolyphaseSynthesizer &b, int noutput_items) {
                 gr_vector_int req(1, 0);
                 b.forecast(noutput_items, req);
                 return req[0];
             },
             py::arg("noutput_items"))
#ifndef MI355_WITH_GNURADIO
        // stand-alone build only: consume_each() outside a flowgraph has nothing to report to
        .def("general_work",
             [](clPolyphaseSynthesizer &b, int noutput_items, const std::vector<py::array> &in, std::vector<py::array> out) {
                 need(noutput_items >= 0, "noutput_items is negative");
                 need(in.size() == 1 && out.size() == 1, "one input and one output");
                 auto i = in_ptrs(in);
                 auto o = out_ptrs(out);
                 gr_vector_int n(1, (int)((size_t)in[0].nbytes() / sizeof(gr_complex)));
                 need((size_t)out[0].nbytes() >= (size_t)noutput_items * sizeof(gr_complex), "output 0 holds fewer than noutput_items items");
                 const long before = b.nitems_consumed(0);
                 const int produced = b.general_work(noutput_items, n, i, o);
                 return py::make_tuple(produced, b.nitems_consumed(0) - before);
             },
             py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"))
#endif
        ;

    // averaged power spectrum (lib/clPowerSpectrum_impl.cc).  general_work() is offered whatever the input array holds and returns
    // (produced, consumed): whole spectra only (vectors of fft_size floats), as under the scheduler.
    py::class_<clPowerSpectrum BLOCK_BASES, std::shared_ptr<clPowerSpectrum>>(m, "clPowerSpectrum")
        .def(py::init(&clPowerSpectrum::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("fft_size"), py::arg("navg"), py::arg("window") = std::vector<float>(), py::arg("hop") = 0, py::arg("shift") = false,
             py::arg("log_output") = false, py::arg("scale") = 1.0f, py::arg("setDebug") = 0)
        .def("fft_size", &clPowerSpectrum::fft_size)
        .def("navg", &clPowerSpectrum::navg)
        .def("hop", &clPowerSpectrum::hop)
        .def("set_scale", &clPowerSpectrum::set_scale, py::arg("scale"))
        .def("set_window", &clPowerSpectrum::set_window, py::arg("window"))
        .def("set_generic", &clPowerSpectrum::set_generic, py::arg("on"))
        .def("route", &clPowerSpectrum::route)
        .def("history", [](clPowerSpectrum &b) { return b.history(); })
        .def("forecast",
             [](clPowerSpectrum &b, int noutput_items) {
                 gr_vector_int req(1, 0);
                 b.forecast(noutput_items, req);
                 return req[0];
             },
             py::arg("noutput_items"))
#ifndef MI355_WITH_GNURADIO
        // stand-alone build only: consume_each() outside a flowgraph has nothing to report to
        .def("general_work",
             [](clPowerSpectrum &b, int noutput_items, const std::vector<py::array> &in, std::vector<py::array> out) {
                 need(noutput_items >= 0, "noutput_items is negative");
                 need(in.size() == 1 && out.size() == 1, "one input and one output");
                 auto i = in_ptrs(in);
                 auto o = out_ptrs(out);
                 gr_vector_int n(1, (int)((size_t)in[0].nbytes() / sizeof(gr_complex)));
                 need((size_t)out[0].nbytes() >= (size_t)noutput_items * sizeof(float) * (size_t)b.fft_size(), "output 0 holds fewer than noutput_items vectors");
                 b.set_offered(n);  // consuming more than the array holds throws
                 const long before = b.nitems_consumed(0);
                 const int produced = b.general_work(noutput_items, n, i, o);
                 return py::make_tuple(produced, b.nitems_consumed(0) - before);
             },
             py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"))
#endif
        ;

    // frequency-translating FIR filter (lib/clFreqXlatingFIRFilter_impl.cc): one output array per centre frequency.  post_freq() is what
    // a message on the "freq" port does (stand-alone build: there is no message passing to deliver one).
    py::class_<clFreqXlatingFIRFilter DECIM_BASES, std::shared_ptr<clFreqXlatingFIRFilter>>(m, "clFreqXlatingFIRFilter")
        .def(py::init(&clFreqXlatingFIRFilter::make), py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"),
             py::arg("decimation"), py::arg("taps"), py::arg("center_freqs"), py::arg("sampling_freq"), py::arg("use_time") = false,
             py::arg("setDebug") = 0)
        .def_static("make_ccc", &clFreqXlatingFIRFilter::make_ccc, py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"),
                    py::arg("devId"), py::arg("decimation"), py::arg("taps"), py::arg("center_freqs"), py::arg("sampling_freq"),
                    py::arg("use_time") = false, py::arg("setDebug") = 0)
        .def("set_center_freq", &clFreqXlatingFIRFilter::set_center_freq, py::arg("center_freq"), py::arg("channel") = 0)
        .def("center_freq", &clFreqXlatingFIRFilter::center_freq, py::arg("channel") = 0)
        .def("taps", &clFreqXlatingFIRFilter::taps)
        .def("set_taps", &clFreqXlatingFIRFilter::set_taps, py::arg("taps"))
        .def("num_channels", &clFreqXlatingFIRFilter::num_channels)
        .def("skip", &clFreqXlatingFIRFilter::skip, py::arg("noutputs"))
        .def("set_generic", &clFreqXlatingFIRFilter::set_generic, py::arg("on"))
        .def("route", &clFreqXlatingFIRFilter::route)
        .def("history", [](clFreqXlatingFIRFilter &b) { return b.history(); })
        .def("decimation", [](clFreqXlatingFIRFilter &b) { return b.decimation(); })
#ifndef MI355_WITH_GNURADIO
        .def("post_freq", [](clFreqXlatingFIRFilter &b, double f) { return b.post_double("freq", f); }, py::arg("freq"))
#endif
        .def("work", &call_work<clFreqXlatingFIRFilter>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // tied-array beamformer (lib/clBeamformer_impl.cc): input items are int8 frames, output items one unit's complex64 / float32 values;
    // weights go in and out as int8 arrays in the layout [f][p][b][s]{re, im}
    using i8array = py::array_t<int8_t, py::array::c_style | py::array::forcecast>;
    py::class_<clBeamformer DECIM_BASES, std::shared_ptr<clBeamformer>>(m, "clBeamformer")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int mode, int polarization, int num_inputs,
                         int num_channels, int num_beams, int integration, bool stokes_i, const i8array &weights, int setDebug) {
                 return clBeamformer::make(openCLPlatformType, devSelector, platformId, devId, mode, polarization, num_inputs, num_channels,
                                           num_beams, integration, stokes_i, std::vector<int8_t>(weights.data(), weights.data() + weights.size()),
                                           setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("mode"),
             py::arg("polarization"), py::arg("num_inputs"), py::arg("num_channels"), py::arg("num_beams"), py::arg("integration") = 1,
             py::arg("stokes_i") = false, py::arg("weights") = i8array(0), py::arg("setDebug") = 0)
        .def("set_weights", [](clBeamformer &b, const i8array &w) { b.set_weights(std::vector<int8_t>(w.data(), w.data() + w.size())); },
             py::arg("weights"))
        .def("set_beam_weights",
             [](clBeamformer &b, int beam, const i8array &w) { b.set_beam_weights(beam, std::vector<int8_t>(w.data(), w.data() + w.size())); },
             py::arg("beam"), py::arg("w_beam"))
        .def("weights",
             [](clBeamformer &b) {
                 const std::vector<int8_t> w = b.weights();
                 return i8array(w.size(), w.data());
             })
        .def("num_beams", &clBeamformer::num_beams)
        .def("frame_bytes", &clBeamformer::frame_bytes)
        .def("out_bytes_per_unit", &clBeamformer::out_bytes_per_unit)
        .def("set_generic", &clBeamformer::set_generic, py::arg("on"))
        .def("route", &clBeamformer::route)
        .def("decimation", [](clBeamformer &b) { return b.decimation(); })
        .def("work", &call_work<clBeamformer>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // F-engine (lib/clFEngine_impl.cc): R complex64 input streams with (P - 1) F items of history in front, output items are int8 frames;
    // taps and gains go in and out as float32 arrays
    using f32array = py::array_t<float, py::array::c_style | py::array::forcecast>;
    py::class_<clFEngine DECIM_BASES, std::shared_ptr<clFEngine>>(m, "clFEngine")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int polarization, int num_inputs, int num_channels,
                         const f32array &taps, int taps_per_channel, bool shift, const f32array &gains, int setDebug) {
                 return clFEngine::make(openCLPlatformType, devSelector, platformId, devId, polarization, num_inputs, num_channels,
                                        std::vector<float>(taps.data(), taps.data() + taps.size()), taps_per_channel, shift,
                                        std::vector<float>(gains.data(), gains.data() + gains.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("polarization"),
             py::arg("num_inputs"), py::arg("num_channels"), py::arg("taps") = f32array(0), py::arg("taps_per_channel") = 1,
             py::arg("shift") = false, py::arg("gains") = f32array(0), py::arg("setDebug") = 0)
        .def("set_gains", [](clFEngine &b, const f32array &g) { b.set_gains(std::vector<float>(g.data(), g.data() + g.size())); }, py::arg("gains"))
        .def("set_input_gain",
             [](clFEngine &b, int input, const f32array &g) { b.set_input_gain(input, std::vector<float>(g.data(), g.data() + g.size())); },
             py::arg("input"), py::arg("gain"))
        .def("gains",
             [](clFEngine &b) {
                 const std::vector<float> g = b.gains();
                 return f32array(g.size(), g.data());
             })
        .def("clips",
             [](clFEngine &b, bool reset) {
                 const std::vector<uint64_t> c = b.clips(reset);
                 return py::array_t<uint64_t>(c.size(), c.data());
             },
             py::arg("reset") = false)
        .def("frame_bytes", &clFEngine::frame_bytes)
        .def("set_generic", &clFEngine::set_generic, py::arg("on"))
        .def("route", &clFEngine::route)
        .def("decimation", [](clFEngine &b) { return b.decimation(); })
        .def("history", [](clFEngine &b) { return b.history(); })
        .def("work", &call_work<clFEngine>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // dedisperser (lib/clDedisperser_impl.cc): input items are time samples of R F floats with max_delay samples of look-ahead behind the
    // call's last output, output items R D floats; the delay table goes in and out as an int32 array
    using i32array = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
    py::class_<clDedisperser SYNC_BASES, std::shared_ptr<clDedisperser>>(m, "clDedisperser")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int num_trials,
                         int max_delay, const i32array &delays, int setDebug) {
                 return clDedisperser::make(openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, num_trials, max_delay,
                                            std::vector<int32_t>(delays.data(), delays.data() + delays.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_rows"),
             py::arg("num_channels"), py::arg("num_trials"), py::arg("max_delay"), py::arg("delays") = i32array(0), py::arg("setDebug") = 0)
        .def("set_delays", [](clDedisperser &b, const i32array &t) { b.set_delays(std::vector<int32_t>(t.data(), t.data() + t.size())); },
             py::arg("delays"))
        .def("delays",
             [](clDedisperser &b) {
                 const std::vector<int32_t> t = b.delays();
                 return i32array(t.size(), t.data());
             })
        .def("max_delay", &clDedisperser::max_delay)
        .def("set_generic", &clDedisperser::set_generic, py::arg("on"))
        .def("route", &clDedisperser::route)
        .def("history", [](clDedisperser &b) { return b.history(); })
        .def("work", &call_work<clDedisperser>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // pulse search (lib/clPulseSearch_impl.cc): input items are time samples of R D floats with 2^(K-1) - 1 samples of look-ahead behind
    // the call's last block, output items the R D peak records of 8 bytes of one block; the statistics go in and out as float arrays
    using f32array = py::array_t<float, py::array::c_style | py::array::forcecast>;
    py::class_<clPulseSearch DECIM_BASES, std::shared_ptr<clPulseSearch>>(m, "clPulseSearch")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_trials, int num_widths,
                         int block_len, const f32array &mean, const f32array &inv_sigma, int setDebug) {
                 return clPulseSearch::make(openCLPlatformType, devSelector, platformId, devId, num_rows, num_trials, num_widths, block_len,
                                            std::vector<float>(mean.data(), mean.data() + mean.size()),
                                            std::vector<float>(inv_sigma.data(), inv_sigma.data() + inv_sigma.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_rows"),
             py::arg("num_trials"), py::arg("num_widths"), py::arg("block_len"), py::arg("mean") = f32array(0),
             py::arg("inv_sigma") = f32array(0), py::arg("setDebug") = 0)
        .def("set_stats",
             [](clPulseSearch &b, const f32array &mean, const f32array &inv_sigma) {
                 b.set_stats(std::vector<float>(mean.data(), mean.data() + mean.size()),
                             std::vector<float>(inv_sigma.data(), inv_sigma.data() + inv_sigma.size()));
             },
             py::arg("mean"), py::arg("inv_sigma"))
        .def("mean",
             [](clPulseSearch &b) {
                 const std::vector<float> t = b.mean();
                 return f32array(t.size(), t.data());
             })
        .def("inv_sigma",
             [](clPulseSearch &b) {
                 const std::vector<float> t = b.inv_sigma();
                 return f32array(t.size(), t.data());
             })
        .def("lookahead", &clPulseSearch::lookahead)
        .def("set_generic", &clPulseSearch::set_generic, py::arg("on"))
        .def("route", &clPulseSearch::route)
        .def("decimation", [](clPulseSearch &b) { return b.decimation(); })
        .def("history", [](clPulseSearch &b) { return b.history(); })
        .def("work", &call_work<clPulseSearch>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // filterbank cleaner (lib/clFilterbankCleaner_impl.cc): items are time samples of R F floats in and out, noutput_items a multiple of
    // block_len; output_items[1] (R bytes per item) and output_items[2] (R F bytes per item) are the optional flag streams
    using u8array = py::array_t<uint8_t, py::array::c_style | py::array::forcecast>;
    py::class_<clFilterbankCleaner SYNC_BASES, std::shared_ptr<clFilterbankCleaner>>(m, "clFilterbankCleaner")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int block_len, double nd,
                         double sk_lo, double sk_hi, double td, bool zero_dm, const u8array &mask, int setDebug) {
                 return clFilterbankCleaner::make(openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, block_len, nd, sk_lo,
                                                  sk_hi, td, zero_dm, std::vector<uint8_t>(mask.data(), mask.data() + mask.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_rows"),
             py::arg("num_channels"), py::arg("block_len"), py::arg("nd") = 1.0, py::arg("sk_lo") = -std::numeric_limits<double>::infinity(),
             py::arg("sk_hi") = std::numeric_limits<double>::infinity(), py::arg("td") = std::numeric_limits<double>::infinity(),
             py::arg("zero_dm") = false, py::arg("mask") = u8array(0), py::arg("setDebug") = 0)
        .def("set_limits", &clFilterbankCleaner::set_limits, py::arg("nd"), py::arg("sk_lo"), py::arg("sk_hi"), py::arg("td"), py::arg("zero_dm"))
        .def("limits", &clFilterbankCleaner::limits)
        .def("set_mask", [](clFilterbankCleaner &b, const u8array &t) { b.set_mask(std::vector<uint8_t>(t.data(), t.data() + t.size())); },
             py::arg("mask"))
        .def("mask",
             [](clFilterbankCleaner &b) {
                 const std::vector<uint8_t> t = b.mask();
                 return u8array(t.size(), t.data());
             })
        .def("block_len", &clFilterbankCleaner::block_len)
        .def("set_generic", &clFilterbankCleaner::set_generic, py::arg("on"))
        .def("route", &clFilterbankCleaner::route)
        .def("output_multiple", [](clFilterbankCleaner &b) { return b.output_multiple(); })
        .def("history", [](clFilterbankCleaner &b) { return b.history(); })
        .def("work", &call_work<clFilterbankCleaner>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // folder (lib/clFolder_impl.cc): input items are time samples of R F floats (input_items[1], optional: R flag bytes per sample), an
    // output item is one sub-integration of R nbin F floats (output_items[1], optional: R nbin uint32 hit counts); models are 3 R uint64
    using u64array = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;
    py::class_<clFolder DECIM_BASES, std::shared_ptr<clFolder>>(m, "clFolder")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int nbin, int subint_len,
                         const u64array &models, int setDebug) {
                 return clFolder::make(openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, nbin, subint_len,
                                       std::vector<uint64_t>(models.data(), models.data() + models.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_rows"),
             py::arg("num_channels"), py::arg("nbin"), py::arg("subint_len"), py::arg("models"), py::arg("setDebug") = 0)
        .def("set_models", [](clFolder &b, const u64array &t) { b.set_models(std::vector<uint64_t>(t.data(), t.data() + t.size())); },
             py::arg("models"))
        .def("models",
             [](clFolder &b) {
                 const std::vector<uint64_t> t = b.models();
                 return u64array(t.size(), t.data());
             })
        .def("sample", &clFolder::sample)
        .def("set_sample", &clFolder::set_sample, py::arg("T"))
        .def("skip", &clFolder::skip, py::arg("n"))
        .def("nbin", &clFolder::nbin)
        .def("subint_len", &clFolder::subint_len)
        .def("set_generic", &clFolder::set_generic, py::arg("on"))
        .def("route", &clFolder::route)
        .def("decimation", [](clFolder &b) { return b.decimation(); })
        .def("history", [](clFolder &b) { return b.history(); })
        .def("work", &call_work<clFolder>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // period search (lib/clPeriodSearch_impl.cc): an input item is one segment of S series of 2^L p_hi floats, an output item its S P 2^L
    // peak records of 8 bytes (output_items[1], optional: the S P 2^L p_hi profile floats)
    py::class_<clPeriodSearch SYNC_BASES, std::shared_ptr<clPeriodSearch>>(m, "clPeriodSearch")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int p_lo, int p_hi, int log2_rows,
                         int num_widths, const f32array &mean, const f32array &inv_sigma, int setDebug) {
                 return clPeriodSearch::make(openCLPlatformType, devSelector, platformId, devId, num_series, p_lo, p_hi, log2_rows, num_widths,
                                             std::vector<float>(mean.data(), mean.data() + mean.size()),
                                             std::vector<float>(inv_sigma.data(), inv_sigma.data() + inv_sigma.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_series"), py::arg("p_lo"),
             py::arg("p_hi"), py::arg("log2_rows"), py::arg("num_widths"), py::arg("mean") = f32array(0), py::arg("inv_sigma") = f32array(0),
             py::arg("setDebug") = 0)
        .def("set_stats",
             [](clPeriodSearch &b, const f32array &mean, const f32array &inv_sigma) {
                 b.set_stats(std::vector<float>(mean.data(), mean.data() + mean.size()),
                             std::vector<float>(inv_sigma.data(), inv_sigma.data() + inv_sigma.size()));
             },
             py::arg("mean"), py::arg("inv_sigma"))
        .def("mean",
             [](clPeriodSearch &b) {
                 const std::vector<float> t = b.mean();
                 return f32array(t.size(), t.data());
             })
        .def("inv_sigma",
             [](clPeriodSearch &b) {
                 const std::vector<float> t = b.inv_sigma();
                 return f32array(t.size(), t.data());
             })
        .def("segment_len", &clPeriodSearch::segment_len)
        .def("records_per_series", &clPeriodSearch::records_per_series)
        .def("period", &clPeriodSearch::period, py::arg("p"), py::arg("i"), py::arg("tsamp_s") = 1.0)
        .def("set_generic", &clPeriodSearch::set_generic, py::arg("on"))
        .def("route", &clPeriodSearch::route)
        .def("history", [](clPeriodSearch &b) { return b.history(); })
        .def("work", &call_work<clPeriodSearch>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // spectral search (lib/clSpectralSearch_impl.cc): an input item is one segment of S series of n floats, an output item its
    // S n / 2 / block_bins peak records of 8 bytes (output_items[1], optional: the S n / 2 spectrum floats)
    py::class_<clSpectralSearch SYNC_BASES, std::shared_ptr<clSpectralSearch>>(m, "clSpectralSearch")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int n, int num_folds, int block_bins,
                         int k_lo, const f32array &inv_sigma, int setDebug) {
                 return clSpectralSearch::make(openCLPlatformType, devSelector, platformId, devId, num_series, n, num_folds, block_bins, k_lo,
                                               std::vector<float>(inv_sigma.data(), inv_sigma.data() + inv_sigma.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_series"), py::arg("n"),
             py::arg("num_folds"), py::arg("block_bins"), py::arg("k_lo") = 1, py::arg("inv_sigma") = f32array(0), py::arg("setDebug") = 0)
        .def("set_stats",
             [](clSpectralSearch &b, const f32array &inv_sigma) {
                 b.set_stats(std::vector<float>(inv_sigma.data(), inv_sigma.data() + inv_sigma.size()));
             },
             py::arg("inv_sigma"))
        .def("inv_sigma",
             [](clSpectralSearch &b) {
                 const std::vector<float> t = b.inv_sigma();
                 return f32array(t.size(), t.data());
             })
        .def("segment_len", &clSpectralSearch::segment_len)
        .def("num_bins", &clSpectralSearch::num_bins)
        .def("records_per_series", &clSpectralSearch::records_per_series)
        .def("freq", &clSpectralSearch::freq, py::arg("h"), py::arg("k"), py::arg("tsamp_s") = 1.0)
        .def("set_generic", &clSpectralSearch::set_generic, py::arg("on"))
        .def("route", &clSpectralSearch::route)
        .def("history", [](clSpectralSearch &b) { return b.history(); })
        .def("work", &call_work<clSpectralSearch>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));

    // acceleration trials (lib/clAccelResampler_impl.cc): an input item is one segment of S series of n floats, an output item its
    // S A resampled series of n floats, [series][trial]
    using i64array = py::array_t<long long, py::array::c_style | py::array::forcecast>;
    py::class_<clAccelResampler SYNC_BASES, std::shared_ptr<clAccelResampler>>(m, "clAccelResampler")
        .def(py::init([](int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int n, const i64array &trials,
                         int setDebug) {
                 return clAccelResampler::make(openCLPlatformType, devSelector, platformId, devId, num_series, n,
                                               std::vector<long long>(trials.data(), trials.data() + trials.size()), setDebug);
             }),
             py::arg("openCLPlatformType"), py::arg("devSelector"), py::arg("platformId"), py::arg("devId"), py::arg("num_series"), py::arg("n"),
             py::arg("trials"), py::arg("setDebug") = 0)
        .def("set_trials",
             [](clAccelResampler &b, const i64array &trials) { b.set_trials(std::vector<long long>(trials.data(), trials.data() + trials.size())); },
             py::arg("trials"))
        .def("trials",
             [](clAccelResampler &b) {
                 const std::vector<long long> t = b.trials();
                 return i64array(t.size(), t.data());
             })
        .def("segment_len", &clAccelResampler::segment_len)
        .def("num_trials", &clAccelResampler::num_trials)
        .def("rows", &clAccelResampler::rows)
        .def("set_generic", &clAccelResampler::set_generic, py::arg("on"))
        .def("route", &clAccelResampler::route)
        .def("history", [](clAccelResampler &b) { return b.history(); })
        .def("work", &call_work<clAccelResampler>, py::arg("noutput_items"), py::arg("input_items"), py::arg("output_items"));
}
