// clPolyphaseSynthesizer_impl: the polyphase synthesis bank over the C ABI (mi355_synth_*).  A general block that works in whole frames:
// nmap items in, num_channels items out, (taps_per_arm - 1) frames of history in front; what a call reads and writes comes from the
// library's own bookkeeping (mi355_synth_plan), so the block and the kernels cannot disagree about a frame.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

class clPolyphaseSynthesizer_impl : public clPolyphaseSynthesizer, BlockBase<mi355_synth, mi355_synth_destroy> {
    const int d_M, d_nmap;

    void apply_history() { set_history((unsigned)((mi355_synth_taps_per_arm(d_h) - 1) * d_nmap + 1)); }

public:
    clPolyphaseSynthesizer_impl(int openCLPlatformType, int devSelector, int platformId, int devId, const std::vector<float> &taps,
                                int num_channels, const std::vector<int> &ch_map, bool setDebug)
        : gr::block("clPolyphaseSynthesizer", gr::io_signature::make(1, 1, (int)sizeof(gr_complex)), gr::io_signature::make(1, 1, (int)sizeof(gr_complex))),
          d_M(num_channels), d_nmap(ch_map.empty() ? num_channels : (int)ch_map.size())
    {
        // argument errors before any device work
        const int rc = mi355_synth_plan((int)taps.size(), num_channels, d_nmap, 0, nullptr, nullptr, nullptr);
        if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(std::string("clPolyphaseSynthesizer: ") + mi355_last_error());
        chk_runtime(rc, "mi355_synth_plan");
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug);
        created(mi355_synth_create(d_ctx, taps.data(), (int)taps.size(), num_channels, ch_map.empty() ? nullptr : ch_map.data(), d_nmap, d_h.adopt()),
                "mi355_synth_create");
        apply_history();
        set_relative_rate((uint64_t)d_M, (uint64_t)d_nmap);
        set_output_multiple(d_M);
    }
    std::vector<float> taps() const override
    {
        const int n = mi355_synth_ntaps(d_h);
        std::vector<float> t((size_t)n);
        chk_runtime(mi355_synth_get_taps(d_h, t.data(), n), "mi355_synth_get_taps");
        return t;
    }
    void set_taps(const std::vector<float> &taps) override
    {
        chk_runtime(mi355_synth_set_taps(d_h, taps.data(), (int)taps.size()), "mi355_synth_set_taps");
        apply_history();
    }
    int taps_per_arm() const override { return mi355_synth_taps_per_arm(d_h); }
    int num_channels() const override { return d_M; }
    int nmap() const override { return d_nmap; }
    std::string route() const override { return mi355_synth_route(d_h); }
    void forecast(int noutput_items, gr_vector_int &req) override
    {
        long long nin = 0;
        chk_runtime(mi355_synth_plan(mi355_synth_ntaps(d_h), d_M, d_nmap, noutput_items / d_M, nullptr, &nin, nullptr), "mi355_synth_plan");
        for (auto &r : req) r = (int)nin;
    }
    // as many whole frames as the offered input and the output room allow: one library call, consume_each(frames x nmap)
    int general_work(int noutput_items, gr_vector_int &ninput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        const long long hist = (long long)(mi355_synth_taps_per_arm(d_h) - 1) * d_nmap;
        long long n = ninput_items[0] >= hist ? (ninput_items[0] - hist) / d_nmap : 0;
        if (n > noutput_items / d_M) n = noutput_items / d_M;
        chk_runtime(mi355_synth_work(d_h, n, in[0], out[0]), "mi355_synth_work");
        consume_each((int)(n * d_nmap));
        return (int)(n * d_M);
    }
};

}  // namespace

clPolyphaseSynthesizer::sptr clPolyphaseSynthesizer::make(int openCLPlatformType, int devSelector, int platformId, int devId,
                                                          const std::vector<float> &taps, int num_channels, const std::vector<int> &ch_map,
                                                          int setDebug)
{
    return sched::adopt(new clPolyphaseSynthesizer_impl(openCLPlatformType, devSelector, platformId, devId, taps, num_channels, ch_map,
                                                        setDebug != 0));
}

}  // namespace clenabled
}  // namespace gr
