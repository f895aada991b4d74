// clRationalResampler_impl: the polyphase interpolating / rational-rate FIR over the C ABI (mi355_resampler_*).  A general block:
// history nt = ceil(ntaps / L), relative rate L / M, forecast() and the number of outputs a call may make both come from the
// library's own bookkeeping (mi355_resampler_plan / _noutput_for), so the block and the kernels cannot disagree about a window.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

class clRationalResampler_impl : public clRationalResampler, BlockBase<mi355_resampler, mi355_resampler_destroy> {
    const int d_interp, d_decim;
    const bool d_complex;

    int phase() const
    {
        int c = 0;
        chk_runtime(mi355_resampler_get_phase(d_h, &c), "mi355_resampler_get_phase");
        return c;
    }
    std::vector<float> flat(const std::vector<gr_complex> &taps) const { return clenabled::flat(taps, d_complex, "clRationalResampler"); }

public:
    clRationalResampler_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int interpolation, int decimation,
                             const std::vector<gr_complex> &taps, bool complex_taps, bool setDebug)
        : gr::block("clRationalResampler", gr::io_signature::make(1, 1, (int)sizeof(gr_complex)), gr::io_signature::make(1, 1, (int)sizeof(gr_complex))),
          d_interp(interpolation), d_decim(decimation), d_complex(complex_taps)
    {
        int nt = 0;  // argument errors before any device work
        const int rc = mi355_resampler_plan(interpolation, decimation, (int)taps.size(), 0, 0, &nt, nullptr, nullptr, nullptr);
        if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(std::string("clRationalResampler: ") + mi355_last_error());
        chk_runtime(rc, "mi355_resampler_plan");
        const std::vector<float> t = flat(taps);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug);
        created(mi355_resampler_create(d_ctx, interpolation, decimation, t.data(), (int)taps.size(), complex_taps ? 1 : 0, d_h.adopt()),
                "mi355_resampler_create", ArgIs::runtime_error);
        set_history(nt);
        set_relative_rate((uint64_t)interpolation, (uint64_t)decimation);
        set_output_multiple(1);
    }
    std::vector<gr_complex> taps() const override
    {
        const int n = mi355_resampler_ntaps(d_h);
        std::vector<float> t((size_t)n * (d_complex ? 2 : 1));
        chk_runtime(mi355_resampler_get_taps(d_h, t.data(), n), "mi355_resampler_get_taps");
        std::vector<gr_complex> out((size_t)n);
        for (int k = 0; k < n; k++) out[k] = d_complex ? gr_complex(t[2 * k], t[2 * k + 1]) : gr_complex(t[k], 0.0f);
        return out;
    }
    void set_taps(const std::vector<gr_complex> &taps) override
    {
        const std::vector<float> t = flat(taps);
        chk_runtime(mi355_resampler_set_taps(d_h, t.data(), (int)taps.size()), "mi355_resampler_set_taps");
        set_history(mi355_resampler_history(d_h));  // the phase is kept
    }
    int interpolation() const override { return d_interp; }
    int decimation() const override { return d_decim; }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        long long needed = 0;
        chk_runtime(mi355_resampler_plan(d_interp, d_decim, mi355_resampler_ntaps(d_h), phase(), noutput_items, nullptr, nullptr, &needed, nullptr),
                    "mi355_resampler_plan");
        for (auto &r : req) r = (int)needed;
    }
    // as many outputs as the offered input allows, at most noutput_items: one library call, consume_each(what it consumed)
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        long long n = mi355_resampler_noutput_for(d_interp, d_decim, mi355_resampler_ntaps(d_h), phase(), ninput_items[0]);
        if (n < 0) chk_runtime((int)n, "mi355_resampler_noutput_for");
        if (n > noutput_items) n = noutput_items;
        long long consumed = 0;
        chk_runtime(mi355_resampler_work(d_h, n, in[0], out[0], &consumed), "mi355_resampler_work");
        consume_each((int)consumed);
        return (int)n;
    }
};

std::vector<gr_complex> widen(const std::vector<float> &taps) { return std::vector<gr_complex>(taps.begin(), taps.end()); }

}  // namespace

clRationalResampler::sptr clRationalResampler::make(int openCLPlatformType, int devSelector, int platformId, int devId, int interpolation,
                                                    int decimation, const std::vector<float> &taps, int setDebug)
{
    return sched::adopt(new clRationalResampler_impl(openCLPlatformType, devSelector, platformId, devId, interpolation, decimation,
                                                     widen(taps), false, setDebug != 0));
}

clRationalResampler::sptr clRationalResampler::make_ccc(int openCLPlatformType, int devSelector, int platformId, int devId, int interpolation,
                                                        int decimation, const std::vector<gr_complex> &taps, int setDebug)
{
    return sched::adopt(new clRationalResampler_impl(openCLPlatformType, devSelector, platformId, devId, interpolation, decimation, taps,
                                                     true, setDebug != 0));
}

}  // namespace clenabled
}  // namespace gr
