// clFolder_impl: exact pulsar folding over the C ABI (mi355_fold_*).  A sync_decimator by subint_len whose input item is one time sample
// of R F floats (with R time-flag bytes on the optional input 1) and whose output item is one sub-integration of R nbin F floats (with R
// nbin hit counts on the optional output 1), so a call for n output items hands the library n subint_len samples.  The models and the
// absolute sample index live in the library handle; the block keeps no stream state.  The "models" message port calls set_models.
#include <clenabled/clenabled.h>
#include <mi355_clenabled.h>

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

void chk(int rc, const char *what)
{
    if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(std::string(what) + ": " + mi355_last_error());
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + mi355_strerror(rc) + ": " + mi355_last_error());
}

struct Plan {
    long long in_floats = 0, out_floats = 0, hits = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int R, int F, int nbin, int Ts)
{
    Plan p;
    chk(mi355_fold_plan(R, F, nbin, Ts, &p.in_floats, &p.out_floats, &p.hits), "clFolder");
    if (p.out_floats * 4 > 0x7fffffffll) throw std::invalid_argument("clFolder: a stream item of 2 GiB or more");
    return p;
}

class clFolder_impl : public clFolder {
    mi355_ctx *d_ctx = nullptr;
    mi355_fold *d_h = nullptr;
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
        chk(mi355_ctx_create(openCLPlatformType, devSelector, platformId, devId, setDebug ? 1 : 0, &d_ctx), "mi355_ctx_create");
        const int rc = mi355_fold_create(d_ctx, R, F, nbin, Ts, models.data(), &d_h);
        if (rc) {
            const std::string msg = std::string("mi355_fold_create: ") + mi355_strerror(rc) + ": " + mi355_last_error();
            mi355_ctx_destroy(d_ctx);
            if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(msg);
            throw std::runtime_error(msg);
        }
#ifdef MI355_WITH_GNURADIO
        message_port_register_in(pmt::mp("models"));
        set_msg_handler(pmt::mp("models"), [this](pmt::pmt_t msg) {
            if (!pmt::is_pair(msg)) return;
            const pmt::pmt_t v = pmt::cdr(msg);
            if (pmt::is_u64vector(v)) post_models(pmt::u64vector_elements(v));
        });
#else
        message_port_register_in("models");
        set_u64vector_handler("models", [this](const std::vector<uint64_t> &m) { post_models(m); });
#endif
    }
    ~clFolder_impl() override
    {
        mi355_fold_destroy(d_h);
        mi355_ctx_destroy(d_ctx);
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
        chk(mi355_fold_set_models(d_h, models.data()), "mi355_fold_set_models");
    }
    std::vector<uint64_t> models() const override
    {
        std::vector<uint64_t> m(d_words);
        chk(mi355_fold_get_models(d_h, m.data(), (long long)m.size()), "mi355_fold_get_models");
        return m;
    }
    uint64_t sample() const override
    {
        unsigned long long T = 0;
        chk(mi355_fold_sample(d_h, &T), "mi355_fold_sample");
        return T;
    }
    void set_sample(uint64_t T) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk(mi355_fold_set_sample(d_h, T), "mi355_fold_set_sample");
    }
    void skip(long long n) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk(mi355_fold_skip(d_h, n), "mi355_fold_skip");
    }
    int nbin() const override { return d_nbin; }
    int subint_len() const override { return d_subint_len; }
    void set_generic(bool on) override { chk(mi355_fold_set_generic(d_h, on ? 1 : 0), "mi355_fold_set_generic"); }
    std::string route() const override { return mi355_fold_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        if (noutput_items <= 0) return 0;
        chk(mi355_fold_work(d_h, (long long)noutput_items * d_subint_len, in[0], in.size() >= 2 ? in[1] : nullptr, out[0],
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
