// clPeriodSearch_impl: exact fast-folding period search over the C ABI (mi355_ffa_*).  A sync_block whose input item is one whole
// segment of S series of 2^L p_hi floats each (series-major, what clDedisperser writes per trial with out_pitch = 2^L p_hi) and whose
// output item is the S P 2^L peak records of that segment; the optional output 1 carries the S P 2^L p_hi profile floats (the floats
// j >= p of a row are left as the scheduler's buffer holds them).  The statistics live in the library handle.
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
    long long n = 0, records = 0, profile_floats = 0, scratch = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int S, int p_lo, int p_hi, int L, int K)
{
    Plan p;
    chk_arg(mi355_ffa_plan(S, p_lo, p_hi, L, K, &p.n, &p.records, &p.profile_floats, &p.scratch), "clPeriodSearch");
    check_stream_item("clPeriodSearch", {p.n * S * 4, p.records * S * 8, p.profile_floats * S * 4});
    return p;
}

class clPeriodSearch_impl : public clPeriodSearch, BlockBase<mi355_ffa, mi355_ffa_destroy> {
    const Plan d_plan;
    const size_t d_series;
    const int d_log2_rows;
    std::mutex d_lock;

    std::vector<float> stats(bool second) const
    {
        std::vector<float> m(d_series), g(d_series);
        chk_arg(mi355_ffa_get_stats(d_h, m.data(), g.data(), (long long)d_series), "mi355_ffa_get_stats");
        return second ? g : m;
    }

public:
    clPeriodSearch_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int S, int p_lo, int p_hi, int L, int K,
                        const std::vector<float> &mean, const std::vector<float> &inv_sigma, bool setDebug, const Plan &p)
        : gr::sync_block("clPeriodSearch", gr::io_signature::make(1, 1, (int)(p.n * S * 4)),
                         gr::io_signature::makev(1, 2, std::vector<int>{(int)(p.records * S * (long long)sizeof(peak)), (int)(p.profile_floats * S * 4)})),
          d_plan(p), d_series((size_t)S), d_log2_rows(L)
    {
        if ((!mean.empty() && mean.size() != d_series) || (!inv_sigma.empty() && inv_sigma.size() != d_series))
            throw std::invalid_argument("clPeriodSearch: mean and inv_sigma hold " + std::to_string(mean.size()) + " and " +
                                        std::to_string(inv_sigma.size()) + " entries, the block has " + std::to_string(d_series) + " series");
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_ffa_create(d_ctx, S, p_lo, p_hi, L, K, mean.empty() ? nullptr : mean.data(), inv_sigma.empty() ? nullptr : inv_sigma.data(),
                                 d_h.adopt()),
                "mi355_ffa_create");
    }
    void set_stats(const std::vector<float> &mean, const std::vector<float> &inv_sigma) override
    {
        if (mean.size() != d_series || inv_sigma.size() != d_series)
            throw std::invalid_argument("clPeriodSearch: set_stats() takes " + std::to_string(d_series) + " entries each, got " +
                                        std::to_string(mean.size()) + " and " + std::to_string(inv_sigma.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_ffa_set_stats(d_h, mean.data(), inv_sigma.data()), "mi355_ffa_set_stats");
    }
    std::vector<float> mean() const override { return stats(false); }
    std::vector<float> inv_sigma() const override { return stats(true); }
    long long segment_len() const override { return d_plan.n; }
    long long records_per_series() const override { return d_plan.records; }
    double period(int p, int i, double tsamp_s) const override { return mi355_ffa_period(p, d_log2_rows, i, tsamp_s); }
    void set_generic(bool on) override { chk_arg(mi355_ffa_set_generic(d_h, on ? 1 : 0), "mi355_ffa_set_generic"); }
    std::string route() const override { return mi355_ffa_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        const size_t in_bytes = (size_t)d_plan.n * d_series * 4, rec_bytes = (size_t)d_plan.records * d_series * sizeof(peak);
        const size_t prof_bytes = (size_t)d_plan.profile_floats * d_series * 4;
        for (int i = 0; i < noutput_items; i++)
            chk_arg(mi355_ffa_work(d_h, (const char *)in[0] + (size_t)i * in_bytes, d_plan.n, (char *)out[0] + (size_t)i * rec_bytes,
                                   out.size() >= 2 ? (char *)out[1] + (size_t)i * prof_bytes : nullptr),
                    "mi355_ffa_work");
        return noutput_items < 0 ? 0 : noutput_items;
    }
};

}  // namespace

clPeriodSearch::sptr clPeriodSearch::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_series, int p_lo, int p_hi,
                                          int log2_rows, int num_widths, const std::vector<float> &mean, const std::vector<float> &inv_sigma,
                                          int setDebug)
{
    const Plan p = plan(num_series, p_lo, p_hi, log2_rows, num_widths);
    return sched::adopt(new clPeriodSearch_impl(openCLPlatformType, devSelector, platformId, devId, num_series, p_lo, p_hi, log2_rows, num_widths,
                                                mean, inv_sigma, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
