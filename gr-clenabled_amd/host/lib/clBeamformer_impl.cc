// clBeamformer_impl: tied-array beamformer on the X-engine's int8 frames over the C ABI (mi355_beamform_*).  A sync_decimator whose
// input item is one frame and whose output item is one unit's output: decimation 1 in VOLTAGE mode, `integration` in POWER mode, so a
// call for n output items hands the library n units = n decimation frames.  Weights live in the library handle.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

struct Plan {
    long long frame_bytes = 0, out_bytes = 0;
    int frames_per_unit = 1;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int mode, int npol, int S, int F, int B, int Ti, bool stokes)
{
    Plan p;
    chk_arg(mi355_beamform_plan(mode, npol, S, F, B, Ti, stokes ? 1 : 0, &p.frame_bytes, &p.frames_per_unit, &p.out_bytes), "clBeamformer");
    check_stream_item("clBeamformer", {p.frame_bytes, p.out_bytes});
    return p;
}

class clBeamformer_impl : public clBeamformer, BlockBase<mi355_beamform, mi355_beamform_destroy> {
    const Plan d_plan;
    const size_t d_wbytes, d_beam_bytes;
    const int d_beams;
    std::mutex d_lock;

public:
    clBeamformer_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int mode, int npol, int S, int F, int B, int Ti,
                      bool stokes, const std::vector<int8_t> &weights, bool setDebug, const Plan &p)
        : gr::sync_decimator("clBeamformer", gr::io_signature::make(1, 1, (int)p.frame_bytes), gr::io_signature::make(1, 1, (int)p.out_bytes),
                             (unsigned)p.frames_per_unit),
          d_plan(p), d_wbytes((size_t)2 * F * npol * B * S), d_beam_bytes((size_t)2 * F * npol * S), d_beams(B)
    {
        if (!weights.empty() && weights.size() != d_wbytes)
            throw std::invalid_argument("clBeamformer: weights hold " + std::to_string(weights.size()) + " bytes, the geometry needs " +
                                        std::to_string(d_wbytes));
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_beamform_create(d_ctx, mode, npol, S, F, B, Ti, stokes ? 1 : 0, weights.empty() ? nullptr : weights.data(), d_h.adopt()),
                "mi355_beamform_create");
    }
    void set_weights(const std::vector<int8_t> &weights) override
    {
        if (weights.size() != d_wbytes)
            throw std::invalid_argument("clBeamformer: set_weights() takes " + std::to_string(d_wbytes) + " bytes, got " + std::to_string(weights.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_beamform_set_weights(d_h, weights.data()), "mi355_beamform_set_weights");
    }
    void set_beam_weights(int beam, const std::vector<int8_t> &w_beam) override
    {
        if (w_beam.size() != d_beam_bytes)
            throw std::invalid_argument("clBeamformer: set_beam_weights() takes " + std::to_string(d_beam_bytes) + " bytes, got " +
                                        std::to_string(w_beam.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_beamform_set_beam_weights(d_h, beam, w_beam.data()), "mi355_beamform_set_beam_weights");
    }
    std::vector<int8_t> weights() const override
    {
        std::vector<int8_t> w(d_wbytes);
        chk_arg(mi355_beamform_get_weights(d_h, w.data(), (long long)w.size()), "mi355_beamform_get_weights");
        return w;
    }
    int num_beams() const override { return d_beams; }
    long long frame_bytes() const override { return d_plan.frame_bytes; }
    long long out_bytes_per_unit() const override { return d_plan.out_bytes; }
    void set_generic(bool on) override { chk_arg(mi355_beamform_set_generic(d_h, on ? 1 : 0), "mi355_beamform_set_generic"); }
    std::string route() const override { return mi355_beamform_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_beamform_work(d_h, noutput_items, in[0], out[0]), "mi355_beamform_work");
        return noutput_items;
    }
};

}  // namespace

clBeamformer::sptr clBeamformer::make(int openCLPlatformType, int devSelector, int platformId, int devId, int mode, int polarization, int num_inputs,
                                      int num_channels, int num_beams, int integration, bool stokes_i, const std::vector<int8_t> &weights,
                                      int setDebug)
{
    const Plan p = plan(mode, polarization, num_inputs, num_channels, num_beams, integration, stokes_i);
    return sched::adopt(new clBeamformer_impl(openCLPlatformType, devSelector, platformId, devId, mode, polarization, num_inputs, num_channels,
                                              num_beams, integration, stokes_i, weights, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
