// clFolder_impl: exact pulsar folding over the C ABI (mi355_fold_*).  A sync_decimator by subint_len whose input item is one time sample
// of R F floats (with R time-flag bytes on the optional input 1) and whose output item is one sub-integration of R nbin F floats (with R
// nbin hit counts on the optional output 1), so a call for n output items hands the library n subint_len samples.  The models and the
// absolute sample index live in the library handle; the block keeps no stream state.  The "models" message port calls set_models.
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
    long long in_floats = 0, out_floats = 0, hits = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int R, int F, int nbin, int Ts)
{
    Plan p;
    chk_arg(mi355_fold_plan(R, F, nbin, Ts, &p.in_floats, &p.out_floats, &p.hits), "clFolder");
    check_stream_item("clFolder", {p.out_floats * 4});
    return p;
}

class clFolder_impl : public clFolder, BlockBase<mi355_fold, mi355_fold_destroy> {
    const Plan d_plan;
    const size_t d_words;
    const int d_nbin, d_subint_len;
    std::mutex d_lock;

public:
    clFolder_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int R, int F, int nbin, int Ts,
                  const std::vector<uint64_t> &models, bool setDebug, const Plan &p)
        : gr::sync_decimator("clFolder", gr::io_signature::makev(1, 2, std::vector<int>{(int)(p.in_floats * 4), R}),
                             gr::io_signature::makev(1, 2, std::vector<int>{(int)(p.out_floats * 4), (int)(p.hits * 4)}), (unsigned)Ts),
          d_plan(p), d_words(3 * (size_t)R), d_nbin(nbin), d_subint_len(Ts)
    {
        if (models.size() != d_words)
            throw std::invalid_argument("clFolder: the models hold " + std::to_string(models.size()) + " words, the geometry has " +
                                        std::to_string(R) + " rows of 3");
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_fold_create(d_ctx, R, F, nbin, Ts, models.data(), d_h.adopt()), "mi355_fold_create");
        sched::register_in_u64vector(this, "models", [this](const std::vector<uint64_t> &m) { post_models(m); });
    }
    // a message of another size is dropped: the scheduler's thread has nobody to throw to
    void post_models(const std::vector<uint64_t> &m)
    {
        if (m.size() == d_words) set_models(m);
    }
    void set_models(const std::vector<uint64_t> &models) override
    {
        if (models.size() != d_words)
            throw std::invalid_argument("clFolder: set_models() takes " + std::to_string(d_words) + " words, got " + std::to_string(models.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fold_set_models(d_h, models.data()), "mi355_fold_set_models");
    }
    std::vector<uint64_t> models() const override
    {
        std::vector<uint64_t> m(d_words);
        chk_arg(mi355_fold_get_models(d_h, m.data(), (long long)m.size()), "mi355_fold_get_models");
        return m;
    }
    uint64_t sample() const override
    {
        unsigned long long T = 0;
        chk_arg(mi355_fold_sample(d_h, &T), "mi355_fold_sample");
        return T;
    }
    void set_sample(uint64_t T) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fold_set_sample(d_h, T), "mi355_fold_set_sample");
    }
    void skip(long long n) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fold_skip(d_h, n), "mi355_fold_skip");
    }
    int nbin() const override { return d_nbin; }
    int subint_len() const override { return d_subint_len; }
    void set_generic(bool on) override { chk_arg(mi355_fold_set_generic(d_h, on ? 1 : 0), "mi355_fold_set_generic"); }
    std::string route() const override { return mi355_fold_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        if (noutput_items <= 0) return 0;
        chk_arg(mi355_fold_work(d_h, (long long)noutput_items * d_subint_len, in[0], in.size() >= 2 ? in[1] : nullptr, out[0],
                                out.size() >= 2 ? out[1] : nullptr),
                "mi355_fold_work");
        return noutput_items;
    }
};

}  // namespace

clFolder::sptr clFolder::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels, int nbin,
                              int subint_len, const std::vector<uint64_t> &models, int setDebug)
{
    const Plan p = plan(num_rows, num_channels, nbin, subint_len);
    return sched::adopt(new clFolder_impl(openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, nbin, subint_len, models,
                                          setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
