// clAccelResampler_impl: exact acceleration trials over the C ABI (mi355_accel_*).  A sync_block whose input item is one whole segment
// of S series of n floats each (series-major, what clDedisperser writes per trial with out_pitch = n) and whose output item is the
// S A resampled series of that segment, [series][trial], each n floats: the input of a clSpectralSearch of S A series.  The trial table
// lives in the library handle.
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
    long long rows = 0, tile = 0, table = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int S, int n, const std::vector<long long> &trials)
{
    Plan p;
    if (trials.size() > 4096) throw std::invalid_argument("clAccelResampler: " + std::to_string(trials.size()) + " trials (at most 4096)");
    chk_arg(mi355_accel_plan(S, n, (int)trials.size(), &p.rows, &p.tile, &p.table), "clAccelResampler");
    check_stream_item("clAccelResampler", {(long long)n * S * 4, p.rows * n * 4});
    return p;
}

class clAccelResampler_impl : public clAccelResampler, BlockBase<mi355_accel, mi355_accel_destroy> {
    const Plan d_plan;
    const size_t d_series, d_trials;
    const int d_n;
    std::mutex d_lock;

public:
    clAccelResampler_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int S, int n, const std::vector<long long> &trials,
                          bool setDebug, const Plan &p)
        : gr::sync_block("clAccelResampler", gr::io_signature::make(1, 1, (int)((long long)n * S * 4)),
                         gr::io_signature::make(1, 1, (int)(p.rows * n * 4))),
          d_plan(p), d_series((size_t)S), d_trials(trials.size()), d_n(n)
    {
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_accel_create(d_ctx, S, n, (int)d_trials, trials.data(), d_h.adopt()), "mi355_accel_create");
    }
    void set_trials(const std::vector<long long> &trials) override
    {
        if (trials.size() != d_trials)
            throw std::invalid_argument("clAccelResampler: set_trials() takes " + std::to_string(d_trials) + " entries, got " +
                                        std::to_string(trials.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_accel_set_trials(d_h, trials.data()), "mi355_accel_set_trials");
    }
    std::vector<long long> trials() const override
    {
        std::vector<long long> c(d_trials);
        chk_arg(mi355_accel_get_trials(d_h, c.data(), (long long)d_trials), "mi355_accel_get_trials");
        return c;
    }
    long long segment_len() const override { return d_n; }
    long long num_trials() const override { return (long long)d_trials; }
    long long rows() const override { return d_plan.rows; }
    void set_generic(bool on) override { chk_arg(mi355_accel_set_generic(d_h, on ? 1 : 0), "mi355_accel_set_generic"); }
    std::string route() const override { return mi355_accel_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        const size_t in_bytes = (size_t)d_n * d_series * 4, out_bytes = (size_t)d_plan.rows * (size_t)d_n * 4;
        for (int i = 0; i < noutput_items; i++)
            chk_arg(mi355_accel_work(d_h, (const char *)in[0] + (size_t)i * in_bytes, d_n, (char *)out[0] + (size_t)i * out_bytes, d_n, 0, (int)d_trials),
                    "mi355_accel_work");
        return noutput_items < 0 ? 0 : noutput_items;
    }
};

}  // namespace

clAccelResampler::sptr clAccelResampler::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int n,
                                              const std::vector<long long> &trials, int setDebug)
{
    const Plan p = plan(num_series, n, trials);
    return sched::adopt(new clAccelResampler_impl(openCLPlatformType, devSelector, platformId, devId, num_series, n, trials, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
