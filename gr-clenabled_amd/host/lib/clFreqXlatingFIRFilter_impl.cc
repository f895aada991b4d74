// clFreqXlatingFIRFilter_impl: tune + FIR + decimate for one or several centre frequencies over the C ABI (mi355_xlate_*).  A
// sync_decimator with one output stream per centre frequency and history ntaps: a call for n outputs hands the library the
// history-prefixed input (n decimation + ntaps - 1 items, what the scheduler guarantees) and the output pointers as they come.  The
// phase of every channel lives in the library handle; the message port "freq" retunes channel 0.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

int streams(const std::vector<double> &freqs) { return freqs.empty() ? 1 : (int)freqs.size(); }

class clFreqXlatingFIRFilter_impl : public clFreqXlatingFIRFilter, BlockBase<mi355_xlate, mi355_xlate_destroy> {
    const int d_nch;
    const bool d_complex;
    std::mutex d_lock;
    bool d_updated = false;

    std::vector<float> flat(const std::vector<gr_complex> &taps) const { return clenabled::flat(taps, d_complex, "clFreqXlatingFIRFilter"); }

public:
    clFreqXlatingFIRFilter_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int decimation, const std::vector<gr_complex> &taps,
                                bool complex_taps, const std::vector<double> &center_freqs, double sampling_freq, bool use_time, bool setDebug)
        : gr::sync_decimator("clFreqXlatingFIRFilter", gr::io_signature::make(1, 1, (int)sizeof(gr_complex)),
                             gr::io_signature::make(streams(center_freqs), streams(center_freqs), (int)sizeof(gr_complex)),
                             (unsigned)(decimation > 0 ? decimation : 1)),
          d_nch((int)center_freqs.size()), d_complex(complex_taps)
    {
        // argument errors before any device work
        chk_arg(mi355_xlate_plan(decimation, (int)taps.size(), 0, nullptr, nullptr), "clFreqXlatingFIRFilter");
        if (center_freqs.empty()) throw std::invalid_argument("clFreqXlatingFIRFilter: at least one centre frequency");
        const std::vector<float> t = flat(taps);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_xlate_create(d_ctx, decimation, t.data(), (int)taps.size(), complex_taps ? 1 : 0, sampling_freq, center_freqs.data(), d_nch,
                                   use_time ? 1 : 0, d_h.adopt()),
                "mi355_xlate_create");
        set_history((unsigned)taps.size());
        sched::register_in_double(this, "freq", [this](double f) { set_center_freq(f, 0); });
    }
    void set_center_freq(double center_freq, int channel) override
    {
        chk_arg(mi355_xlate_set_center_freq(d_h, channel, center_freq), "mi355_xlate_set_center_freq");
    }
    double center_freq(int channel) const override
    {
        double f = 0.0;
        chk_arg(mi355_xlate_get_center_freq(d_h, channel, &f), "mi355_xlate_get_center_freq");
        return f;
    }
    std::vector<gr_complex> taps() const override
    {
        const int n = mi355_xlate_ntaps(d_h);
        std::vector<float> t((size_t)n * (d_complex ? 2 : 1));
        chk_arg(mi355_xlate_get_taps(d_h, t.data(), n), "mi355_xlate_get_taps");
        std::vector<gr_complex> out((size_t)n);
        for (int k = 0; k < n; k++) out[k] = d_complex ? gr_complex(t[2 * k], t[2 * k + 1]) : gr_complex(t[k], 0.0f);
        return out;
    }
    void set_taps(const std::vector<gr_complex> &taps) override
    {
        const std::vector<float> t = flat(taps);
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_xlate_set_taps(d_h, t.data(), (int)taps.size()), "mi355_xlate_set_taps");
        d_updated = true;
    }
    int num_channels() const override { return d_nch; }
    void skip(long long noutputs) override { chk_arg(mi355_xlate_skip(d_h, noutputs), "mi355_xlate_skip"); }
    void set_generic(bool on) override { chk_arg(mi355_xlate_set_generic(d_h, on ? 1 : 0), "mi355_xlate_set_generic"); }
    std::string route() const override { return mi355_xlate_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        if (d_updated) {  // new taps: the new history first, nothing produced this call (the input on offer was sized for the old one)
            set_history((unsigned)mi355_xlate_ntaps(d_h));
            d_updated = false;
            return 0;
        }
        if ((int)out.size() < d_nch) throw std::logic_error("clFreqXlatingFIRFilter: fewer output streams than centre frequencies");
        chk_arg(mi355_xlate_work(d_h, noutput_items, in[0], out.data()), "mi355_xlate_work");
        return noutput_items;
    }
};

std::vector<gr_complex> widen(const std::vector<float> &taps) { return std::vector<gr_complex>(taps.begin(), taps.end()); }

}  // namespace

clFreqXlatingFIRFilter::sptr clFreqXlatingFIRFilter::make(int openCLPlatformType, int devSelector, int platformId, int devId, int decimation,
                                                          const std::vector<float> &taps, const std::vector<double> &center_freqs,
                                                          double sampling_freq, bool use_time, int setDebug)
{
    return sched::adopt(new clFreqXlatingFIRFilter_impl(openCLPlatformType, devSelector, platformId, devId, decimation, widen(taps), false, center_freqs,
                                                        sampling_freq, use_time, setDebug != 0));
}

clFreqXlatingFIRFilter::sptr clFreqXlatingFIRFilter::make_ccc(int openCLPlatformType, int devSelector, int platformId, int devId, int decimation,
                                                              const std::vector<gr_complex> &taps, const std::vector<double> &center_freqs,
                                                              double sampling_freq, bool use_time, int setDebug)
{
    return sched::adopt(new clFreqXlatingFIRFilter_impl(openCLPlatformType, devSelector, platformId, devId, decimation, taps, true, center_freqs,
                                                        sampling_freq, use_time, setDebug != 0));
}

}  // namespace clenabled
}  // namespace gr
