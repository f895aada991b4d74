// clFEngine_impl: polyphase filter bank + DFT + int8 quantisation into the X-engine's frames over the C ABI (mi355_fengine_*).  A
// sync_decimator over R complex inputs whose output item is one frame: decimation num_channels, history (P - 1) num_channels + 1, so
// a call for n output items hands the library, per input, the n num_channels new items with (P - 1) num_channels items in front.
// Taps, gains and the clip counters live in the library handle.
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
    long long frame_bytes = 0, history_items = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int npol, int S, int F, int P, bool shift)
{
    Plan p;
    chk_arg(mi355_fengine_plan(S, npol, F, P, shift ? 1 : 0, 0, &p.frame_bytes, &p.history_items, nullptr), "clFEngine");
    if (p.frame_bytes > 0x7fffffffll || p.history_items >= 0x7fffffffll) throw std::invalid_argument("clFEngine: a stream item or a history of 2 GiB or more");
    return p;
}

class clFEngine_impl : public clFEngine, BlockBase<mi355_fengine, mi355_fengine_destroy> {
    const Plan d_plan;
    const int d_nin, d_nchan;
    std::mutex d_lock;

public:
    clFEngine_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int npol, int S, int F, const std::vector<float> &taps,
                   int P, bool shift, const std::vector<float> &gains, bool setDebug, const Plan &p)
        : gr::sync_decimator("clFEngine", gr::io_signature::make(S * npol, S * npol, sizeof(gr_complex)),
                             gr::io_signature::make(1, 1, (int)p.frame_bytes), (unsigned)F),
          d_plan(p), d_nin(S * npol), d_nchan(F)
    {
        if (!taps.empty() && taps.size() != (size_t)P * F)
            throw std::invalid_argument("clFEngine: taps hold " + std::to_string(taps.size()) + " values, the geometry needs " +
                                        std::to_string((size_t)P * F));
        if (!gains.empty() && gains.size() != (size_t)d_nin * F)
            throw std::invalid_argument("clFEngine: gains hold " + std::to_string(gains.size()) + " values, the geometry needs " +
                                        std::to_string((size_t)d_nin * F));
        set_history((unsigned)p.history_items + 1);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_fengine_create(d_ctx, S, npol, F, P, taps.empty() ? nullptr : taps.data(), shift ? 1 : 0,
                                     gains.empty() ? nullptr : gains.data(), d_h.adopt()),
                "mi355_fengine_create");
    }
    void set_gains(const std::vector<float> &gains) override
    {
        if (gains.size() != (size_t)d_nin * d_nchan)
            throw std::invalid_argument("clFEngine: set_gains() takes " + std::to_string((size_t)d_nin * d_nchan) + " values, got " +
                                        std::to_string(gains.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fengine_set_gains(d_h, gains.data()), "mi355_fengine_set_gains");
    }
    void set_input_gain(int input, const std::vector<float> &gain) override
    {
        if (gain.size() != (size_t)d_nchan)
            throw std::invalid_argument("clFEngine: set_input_gain() takes " + std::to_string(d_nchan) + " values, got " + std::to_string(gain.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fengine_set_input_gain(d_h, input, gain.data()), "mi355_fengine_set_input_gain");
    }
    std::vector<float> gains() const override
    {
        std::vector<float> g((size_t)d_nin * d_nchan);
        chk_arg(mi355_fengine_get_gains(d_h, g.data(), (long long)g.size()), "mi355_fengine_get_gains");
        return g;
    }
    std::vector<uint64_t> clips(bool reset) override
    {
        std::vector<unsigned long long> c((size_t)d_nin);
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fengine_get_clips(d_h, c.data(), reset ? 1 : 0), "mi355_fengine_get_clips");
        return std::vector<uint64_t>(c.begin(), c.end());
    }
    long long frame_bytes() const override { return d_plan.frame_bytes; }
    void set_generic(bool on) override { chk_arg(mi355_fengine_set_generic(d_h, on ? 1 : 0), "mi355_fengine_set_generic"); }
    std::string route() const override { return mi355_fengine_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fengine_work(d_h, noutput_items, in.data(), out[0]), "mi355_fengine_work");
        return noutput_items;
    }
};

}  // namespace

clFEngine::sptr clFEngine::make(int openCLPlatformType, int devSelector, int platformId, int devId, int polarization, int num_inputs,
                                int num_channels, const std::vector<float> &taps, int taps_per_channel, bool shift,
                                const std::vector<float> &gains, int setDebug)
{
    const Plan p = plan(polarization, num_inputs, num_channels, taps_per_channel, shift);
    return sched::adopt(new clFEngine_impl(openCLPlatformType, devSelector, platformId, devId, polarization, num_inputs, num_channels, taps,
                                           taps_per_channel, shift, gains, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
