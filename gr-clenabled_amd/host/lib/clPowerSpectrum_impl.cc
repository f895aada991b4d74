// clPowerSpectrum_impl: the averaged power spectrum over the C ABI (mi355_pspec_*).  A general block from complex items to vectors of
// fft_size floats: a spectrum needs (navg - 1) hop + fft_size items and consumes navg hop of them; what a call reads and writes comes from
// the library's own bookkeeping (mi355_pspec_plan), so the block and the kernels cannot disagree about a frame.  With hop > fft_size the
// items consumed reach past the last frame read: the block then waits until the scheduler offers all navg hop items of a spectrum, so
// that it never consumes more than it was offered (the library is still handed, and reads, only (S navg - 1) hop + fft_size items).
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

class clPowerSpectrum_impl : public clPowerSpectrum, BlockBase<mi355_pspec, mi355_pspec_destroy> {
    const int d_N, d_K, d_H;

public:
    clPowerSpectrum_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int fft_size, int navg, const std::vector<float> &window,
                         int hop, bool shift, bool log_output, float scale, bool setDebug)
        : gr::block("clPowerSpectrum", gr::io_signature::make(1, 1, (int)sizeof(gr_complex)),
                    gr::io_signature::make(1, 1, (int)sizeof(float) * (fft_size > 0 ? fft_size : 1))),
          d_N(fft_size), d_K(navg), d_H(hop == 0 ? fft_size : hop)
    {
        // argument errors before any device work
        const int rc = mi355_pspec_plan(d_N, d_K, d_H, 0, nullptr, nullptr);
        if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(std::string("clPowerSpectrum: ") + mi355_last_error());
        chk_runtime(rc, "mi355_pspec_plan");
        if (!window.empty() && (int)window.size() != d_N) throw std::invalid_argument("clPowerSpectrum: window not the same length as fft_size");
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug);
        created(mi355_pspec_create(d_ctx, d_N, window.empty() ? nullptr : window.data(), (int)window.size(), d_K, d_H, shift ? 1 : 0,
                                   log_output ? 1 : 0, scale, d_h.adopt()),
                "mi355_pspec_create");
        set_history((unsigned)((d_N > d_H ? d_N - d_H : 0) + 1));
        set_relative_rate((uint64_t)1, (uint64_t)d_K * (uint64_t)d_H);
    }
    int fft_size() const override { return d_N; }
    int navg() const override { return d_K; }
    int hop() const override { return d_H; }
    void set_scale(float scale) override { chk_runtime(mi355_pspec_set_scale(d_h, scale), "mi355_pspec_set_scale"); }
    void set_window(const std::vector<float> &window) override
    {
        if (!window.empty() && (int)window.size() != d_N) throw std::invalid_argument("clPowerSpectrum: window not the same length as fft_size");
        chk_runtime(mi355_pspec_set_window(d_h, window.empty() ? nullptr : window.data(), (int)window.size()), "mi355_pspec_set_window");
    }
    void set_generic(bool on) override { chk_runtime(mi355_pspec_set_generic(d_h, on ? 1 : 0), "mi355_pspec_set_generic"); }
    std::string route() const override { return mi355_pspec_route(d_h); }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        long long nin = 0;
        chk_runtime(mi355_pspec_plan(d_N, d_K, d_H, noutput_items, &nin, nullptr), "mi355_pspec_plan");
        const long long used = (long long)noutput_items * d_K * d_H;  // what general_work() will consume: more than it reads when hop > fft_size
        for (auto &r : req) r = (int)(nin > used ? nin : used);
    }
    // as many whole spectra as the offered input and the output room allow: one library call, consume_each(spectra x navg x hop)
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        const long long have = ninput_items[0];
        long long n = have >= d_N ? ((have - d_N) / d_H + 1) / d_K : 0;  // frames that fit, in whole spectra
        if (d_H > d_N) n = have / ((long long)d_K * d_H);                // ... and whose skipped items were offered too
        if (n > noutput_items) n = noutput_items;
        chk_runtime(mi355_pspec_work(d_h, n, in[0], out[0]), "mi355_pspec_work");
        consume_each((int)(n * d_K * d_H));
        return (int)n;
    }
};

}  // namespace

clPowerSpectrum::sptr clPowerSpectrum::make(int openCLPlatformType, int devSelector, int platformId, int devId, int fft_size, int navg,
                                            const std::vector<float> &window, int hop, bool shift, bool log_output, float scale, int setDebug)
{
    return sched::adopt(new clPowerSpectrum_impl(openCLPlatformType, devSelector, platformId, devId, fft_size, navg, window, hop, shift, log_output,
                                                 scale, setDebug != 0));
}

}  // namespace clenabled
}  // namespace gr
