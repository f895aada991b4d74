// clDedisperser_impl: exact incoherent dedispersion over the C ABI (mi355_dedisp_*).  A sync_block whose input item is one time sample
// of R F floats and whose output item is that sample's R D sums (TIME_MAJOR); history max_delay + 1, so a call for n output items hands
// the library the n samples with max_delay samples of look-ahead behind them.  The delay table lives in the library handle.
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
    long long in_floats = 0, history = 0, out_floats = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int R, int F, int D, int H)
{
    Plan p;
    chk_arg(mi355_dedisp_plan(R, F, D, H, MI355_DEDISP_TIME_MAJOR, &p.in_floats, &p.history, &p.out_floats), "clDedisperser");
    check_stream_item("clDedisperser", {p.in_floats * 4, p.out_floats * 4});
    return p;
}

class clDedisperser_impl : public clDedisperser, BlockBase<mi355_dedisp, mi355_dedisp_destroy> {
    const Plan d_plan;
    const size_t d_entries;
    std::mutex d_lock;

public:
    clDedisperser_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int R, int F, int D, int H,
                       const std::vector<int32_t> &delays, bool setDebug, const Plan &p)
        : gr::sync_block("clDedisperser", gr::io_signature::make(1, 1, (int)(p.in_floats * 4)), gr::io_signature::make(1, 1, (int)(p.out_floats * 4))),
          d_plan(p), d_entries((size_t)D * F)
    {
        if (!delays.empty() && delays.size() != d_entries)
            throw std::invalid_argument("clDedisperser: delays hold " + std::to_string(delays.size()) + " entries, the geometry needs " +
                                        std::to_string(d_entries));
        set_history((unsigned)p.history + 1);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_dedisp_create(d_ctx, R, F, D, H, MI355_DEDISP_TIME_MAJOR, delays.empty() ? nullptr : delays.data(), d_h.adopt()),
                "mi355_dedisp_create");
    }
    void set_delays(const std::vector<int32_t> &delays) override
    {
        if (delays.size() != d_entries)
            throw std::invalid_argument("clDedisperser: set_delays() takes " + std::to_string(d_entries) + " entries, got " + std::to_string(delays.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_dedisp_set_delays(d_h, delays.data()), "mi355_dedisp_set_delays");
    }
    std::vector<int32_t> delays() const override
    {
        std::vector<int32_t> t(d_entries);
        chk_arg(mi355_dedisp_get_delays(d_h, t.data(), (long long)t.size()), "mi355_dedisp_get_delays");
        return t;
    }
    int max_delay() const override { return (int)d_plan.history; }
    void set_generic(bool on) override { chk_arg(mi355_dedisp_set_generic(d_h, on ? 1 : 0), "mi355_dedisp_set_generic"); }
    std::string route() const override { return mi355_dedisp_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_dedisp_work(d_h, noutput_items, in[0], out[0], 0), "mi355_dedisp_work");
        return noutput_items;
    }
};

}  // namespace

clDedisperser::sptr clDedisperser::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels,
                                        int num_trials, int max_delay, const std::vector<int32_t> &delays, int setDebug)
{
    const Plan p = plan(num_rows, num_channels, num_trials, max_delay);
    return sched::adopt(new clDedisperser_impl(openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, num_trials, max_delay,
                                               delays, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
