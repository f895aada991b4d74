// clSpectralSearch_impl: FFT periodicity search with exact harmonic sums over the C ABI (mi355_ssearch_*), SERIES input.  A sync_block
// whose input item is one whole segment of S series of n floats each (series-major, what clDedisperser writes per trial with
// out_pitch = n) and whose output item is the S n / 2 / block_bins peak records of that segment; the optional output 1 carries the
// S n / 2 spectrum floats.  The statistics live in the library handle.  Candidates are not exposed here: there is no message port.
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
    long long bins = 0, records = 0, scratch = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int S, int n, int H, int Bb, int k_lo)
{
    Plan p;
    chk_arg(mi355_ssearch_plan(S, n, H, Bb, k_lo, MI355_SSEARCH_SERIES, &p.bins, &p.records, &p.scratch), "clSpectralSearch");
    check_stream_item("clSpectralSearch", {(long long)n * S * 4, p.records * S * 8, p.bins * S * 4});
    return p;
}

class clSpectralSearch_impl : public clSpectralSearch, BlockBase<mi355_ssearch, mi355_ssearch_destroy> {
    const Plan d_plan;
    const size_t d_series;
    const int d_n;
    std::mutex d_lock;

public:
    clSpectralSearch_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int S, int n, int H, int Bb, int k_lo,
                          const std::vector<float> &inv_sigma, bool setDebug, const Plan &p)
        : gr::sync_block("clSpectralSearch", gr::io_signature::make(1, 1, (int)((long long)n * S * 4)),
                         gr::io_signature::makev(1, 2, std::vector<int>{(int)(p.records * S * (long long)sizeof(peak)), (int)(p.bins * S * 4)})),
          d_plan(p), d_series((size_t)S), d_n(n)
    {
        if (!inv_sigma.empty() && inv_sigma.size() != d_series)
            throw std::invalid_argument("clSpectralSearch: inv_sigma holds " + std::to_string(inv_sigma.size()) + " entries, the block has " +
                                        std::to_string(d_series) + " series");
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_ssearch_create(d_ctx, S, n, H, Bb, k_lo, MI355_SSEARCH_SERIES, inv_sigma.empty() ? nullptr : inv_sigma.data(), d_h.adopt()),
                "mi355_ssearch_create");
    }
    void set_stats(const std::vector<float> &inv_sigma) override
    {
        if (inv_sigma.size() != d_series)
            throw std::invalid_argument("clSpectralSearch: set_stats() takes " + std::to_string(d_series) + " entries, got " +
                                        std::to_string(inv_sigma.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_ssearch_set_stats(d_h, inv_sigma.data()), "mi355_ssearch_set_stats");
    }
    std::vector<float> inv_sigma() const override
    {
        std::vector<float> g(d_series);
        chk_arg(mi355_ssearch_get_stats(d_h, g.data(), (long long)d_series), "mi355_ssearch_get_stats");
        return g;
    }
    long long segment_len() const override { return d_n; }
    long long num_bins() const override { return d_plan.bins; }
    long long records_per_series() const override { return d_plan.records; }
    double freq(int h, int k, double tsamp_s) const override { return mi355_ssearch_freq(d_n, tsamp_s, h, k); }
    void set_generic(bool on) override { chk_arg(mi355_ssearch_set_generic(d_h, on ? 1 : 0), "mi355_ssearch_set_generic"); }
    std::string route() const override { return mi355_ssearch_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        const size_t in_bytes = (size_t)d_n * d_series * 4, rec_bytes = (size_t)d_plan.records * d_series * sizeof(peak);
        const size_t spec_bytes = (size_t)d_plan.bins * d_series * 4;
        for (int i = 0; i < noutput_items; i++)
            chk_arg(mi355_ssearch_work(d_h, (const char *)in[0] + (size_t)i * in_bytes, d_n, (char *)out[0] + (size_t)i * rec_bytes,
                                       out.size() >= 2 ? (char *)out[1] + (size_t)i * spec_bytes : nullptr, nullptr, 0, nullptr),
                    "mi355_ssearch_work");
        return noutput_items < 0 ? 0 : noutput_items;
    }
};

}  // namespace

clSpectralSearch::sptr clSpectralSearch::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int n,
                                              int num_folds, int block_bins, int k_lo, const std::vector<float> &inv_sigma, int setDebug)
{
    const Plan p = plan(num_series, n, num_folds, block_bins, k_lo);
    return sched::adopt(new clSpectralSearch_impl(openCLPlatformType, devSelector, platformId, devId, num_series, n, num_folds, block_bins, k_lo,
                                                  inv_sigma, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
