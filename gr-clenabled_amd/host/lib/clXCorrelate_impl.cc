// clXCorrelate_impl: the reference's lib/clXCorrelate_impl.cc over the C ABI (mi355_xcorr_td_*).  work() keeps the reference's
// frame contract (:1529-1645): one frame of signal_length items per call, decimation counter starting at 1, and in async mode
// submit-and-return with the previous result published when the next frame is accepted; the handle's stream stands in for the
// reference's worker thread.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

class clXCorrelate_impl : public clXCorrelate, BlockBase<mi355_xcorr_td, mi355_xcorr_td_destroy> {
    const int d_num_inputs, d_signal_length, d_decim_frames;
    const bool d_async;
    int cur_frame_counter = 1;   // :708
    bool d_pending = false;      // a submission not collected yet
    bool d_have_result = false;  // a collected result waiting for the next accepted frame
    std::vector<float> d_corr;
    std::vector<int32_t> d_lags;
    std::mutex d_mutex;

    bool take_frame()  // :1539-1546 / :1607-1615
    {
        if (d_decim_frames > 1) {
            if ((cur_frame_counter++ % d_decim_frames) == 0) cur_frame_counter = 1;
            else return false;
        }
        return true;
    }
    void publish() { sched::publish_corr_pdu(this, "corr", d_corr, d_lags); }  // :1594-1600

public:
    clXCorrelate_impl(int openCLPlatformType, int devSelector, int platformId, int devId, bool setDebug, int num_inputs,
                      int signal_length, int data_type, int data_size, int max_search_index, int decim_frames, bool async)
        : gr::sync_block("clXCorrelate", gr::io_signature::make(2, num_inputs, data_size), gr::io_signature::make(0, 0, 0)),  // :704-705
          d_num_inputs(num_inputs), d_signal_length(signal_length), d_decim_frames(decim_frames), d_async(async),
          d_corr(num_inputs > 1 ? num_inputs - 1 : 1), d_lags(num_inputs > 1 ? num_inputs - 1 : 1)
    {
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug);
        created(mi355_xcorr_td_create(d_ctx, num_inputs, signal_length, data_type, data_size, max_search_index, d_h.adopt()), "mi355_xcorr_td_create",
                ArgIs::runtime_error);  // (the reference exit(1)s)
        set_output_multiple(signal_length);  // :839
        sched::register_out(this, "corr");
    }
    // (at destruction a result still pending is dropped, as at the reference's stop())
    int max_shift() const override { return mi355_xcorr_td_max_shift(d_h); }
    int signal_length() const override { return d_signal_length; }
    void wait() override { chk_runtime(mi355_xcorr_td_wait(d_h), "mi355_xcorr_td_wait"); }

    int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &) override
    {
        if (noutput_items < d_signal_length) return 0;
        if ((int)input_items.size() < d_num_inputs) throw std::invalid_argument("clXCorrelate: fewer inputs connected than num_inputs");
        std::lock_guard<std::mutex> guard(d_mutex);
        if (!d_async) {
            if (!take_frame()) return d_signal_length;
            chk_runtime(mi355_xcorr_td_work(d_h, input_items.data(), d_corr.data(), d_lags.data()), "mi355_xcorr_td_work");
            publish();
            return d_signal_length;
        }
        if (d_pending) {
            const int r = mi355_xcorr_td_poll(d_h, d_corr.data(), d_lags.data());
            chk_runtime(r, "mi355_xcorr_td_poll");
            if (r == 0) return d_signal_length;  // still running: the frame passes through, uncounted
            d_pending = false;
            d_have_result = true;
        }
        if (!take_frame()) return d_signal_length;
        if (d_have_result) {  // nothing for the first submission
            publish();
            d_have_result = false;
        }
        chk_runtime(mi355_xcorr_td_submit(d_h, input_items.data()), "mi355_xcorr_td_submit");
        d_pending = true;
        return d_signal_length;
    }
};

}  // namespace

clXCorrelate::sptr clXCorrelate::make(int openCLPlatformType, int devSelector, int platformId, int devId, bool setDebug, int num_inputs,
                                      int signal_length, int data_type, int data_size, int max_search_index, int decim_frames, bool async)
{
    return sched::adopt(new clXCorrelate_impl(openCLPlatformType, devSelector, platformId, devId, setDebug, num_inputs, signal_length,
                                              data_type, data_size, max_search_index, decim_frames, async));
}

}  // namespace clenabled
}  // namespace gr
