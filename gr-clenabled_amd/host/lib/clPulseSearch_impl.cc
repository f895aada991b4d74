// clPulseSearch_impl: exact boxcar single-pulse search over the C ABI (mi355_psearch_*).  A sync_decimator by block_len whose input item
// is one time sample of R D floats (TIME_MAJOR, what clDedisperser writes) and whose output item is the R D peak records of one block;
// history 2^(K-1), so a call for n output items hands the library n block_len samples with 2^(K-1) - 1 samples of look-ahead behind
// them.  The statistics live in the library handle.  Candidates are not exposed here: there is no message port.
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
    long long in_floats = 0, history = 0, peaks = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int R, int D, int K, int Tb)
{
    Plan p;
    chk_arg(mi355_psearch_plan(R, D, K, Tb, MI355_PSEARCH_TIME_MAJOR, &p.in_floats, &p.history, &p.peaks), "clPulseSearch");
    return p;
}

class clPulseSearch_impl : public clPulseSearch, BlockBase<mi355_psearch, mi355_psearch_destroy> {
    const Plan d_plan;
    const size_t d_series;
    const int d_block_len;
    std::mutex d_lock;

    std::vector<float> stats(bool second) const
    {
        std::vector<float> m(d_series), g(d_series);
        chk_arg(mi355_psearch_get_stats(d_h, m.data(), g.data(), (long long)d_series), "mi355_psearch_get_stats");
        return second ? g : m;
    }

public:
    clPulseSearch_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int R, int D, int K, int Tb, const std::vector<float> &mean,
                       const std::vector<float> &inv_sigma, bool setDebug, const Plan &p)
        : gr::sync_decimator("clPulseSearch", gr::io_signature::make(1, 1, (int)(p.in_floats * 4)),
                             gr::io_signature::make(1, 1, (int)(p.peaks * (long long)sizeof(peak))), (unsigned)Tb),
          d_plan(p), d_series((size_t)R * D), d_block_len(Tb)
    {
        if ((!mean.empty() && mean.size() != d_series) || (!inv_sigma.empty() && inv_sigma.size() != d_series))
            throw std::invalid_argument("clPulseSearch: mean and inv_sigma hold " + std::to_string(mean.size()) + " and " +
                                        std::to_string(inv_sigma.size()) + " entries, the geometry has " + std::to_string(d_series) + " series");
        set_history((unsigned)p.history + 1);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_psearch_create(d_ctx, R, D, K, Tb, MI355_PSEARCH_TIME_MAJOR, mean.empty() ? nullptr : mean.data(),
                                     inv_sigma.empty() ? nullptr : inv_sigma.data(), d_h.adopt()),
                "mi355_psearch_create");
    }
    void set_stats(const std::vector<float> &mean, const std::vector<float> &inv_sigma) override
    {
        if (mean.size() != d_series || inv_sigma.size() != d_series)
            throw std::invalid_argument("clPulseSearch: set_stats() takes " + std::to_string(d_series) + " entries each, got " +
                                        std::to_string(mean.size()) + " and " + std::to_string(inv_sigma.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_psearch_set_stats(d_h, mean.data(), inv_sigma.data()), "mi355_psearch_set_stats");
    }
    std::vector<float> mean() const override { return stats(false); }
    std::vector<float> inv_sigma() const override { return stats(true); }
    int lookahead() const override { return (int)d_plan.history; }
    void set_generic(bool on) override { chk_arg(mi355_psearch_set_generic(d_h, on ? 1 : 0), "mi355_psearch_set_generic"); }
    std::string route() const override { return mi355_psearch_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_psearch_work(d_h, (long long)noutput_items * d_block_len, in[0], 0, out[0], nullptr, 0, nullptr), "mi355_psearch_work");
        return noutput_items;
    }
};

}  // namespace

clPulseSearch::sptr clPulseSearch::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_trials,
                                        int num_widths, int block_len, const std::vector<float> &mean, const std::vector<float> &inv_sigma, int setDebug)
{
    const Plan p = plan(num_rows, num_trials, num_widths, block_len);
    return sched::adopt(new clPulseSearch_impl(openCLPlatformType, devSelector, platformId, devId, num_rows, num_trials, num_widths, block_len, mean,
                                               inv_sigma, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
