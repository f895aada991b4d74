// clCostasLoop_impl: the reference's lib/clCostasLoop_impl.cc over the C ABI (mi355_costas_*), one stream.  The loop state (phase,
// frequency, error) lives on the device and carries from one work() call to the next (:525-596); the getters read it back.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

class clCostasLoop_impl : public clCostasLoop, BlockBase<mi355_costas, mi355_costas_destroy> {
    const int d_order;
    float d_loop_bw, d_alpha = 0, d_beta = 0;

    void plan(float bw)  // the reference's invalid_argument (:80-83), before any device work
    {
        const int rc = mi355_costas_plan(bw, d_order, &d_alpha, &d_beta);
        if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(std::string("clCostasLoop: ") + mi355_last_error());
        chk_runtime(rc, "mi355_costas_plan");
        d_loop_bw = bw;
    }

public:
    clCostasLoop_impl(int openCLPlatformType, int devSelector, int platformId, int devId, float loop_bw, int order, bool setDebug)
        : gr::sync_block("clCostasLoop", gr::io_signature::make(1, 1, sizeof(gr_complex)),
                         gr::io_signature::makev(1, 2, std::vector<int>{(int)sizeof(gr_complex), (int)sizeof(float)})),  // :56-57, :456-458
          d_order(order), d_loop_bw(loop_bw)
    {
        plan(loop_bw);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug);
        created(mi355_costas_create(d_ctx, loop_bw, order, 1, d_h.adopt()), "mi355_costas_create", ArgIs::runtime_error);
    }
    void set_loop_bandwidth(float bw) override
    {
        plan(bw);
        chk_runtime(mi355_costas_set_loop_bandwidth(d_h, bw), "mi355_costas_set_loop_bandwidth");
    }
    float get_loop_bandwidth() const override { return d_loop_bw; }
    float get_alpha() const override { return d_alpha; }
    float get_beta() const override { return d_beta; }
    float get_frequency() const override
    {
        double v = 0;
        chk_runtime(mi355_costas_get_state(d_h, nullptr, &v, nullptr), "mi355_costas_get_state");
        return (float)v;
    }
    float get_phase() const override
    {
        double v = 0;
        chk_runtime(mi355_costas_get_state(d_h, &v, nullptr, nullptr), "mi355_costas_get_state");
        return (float)v;
    }
    void set_frequency(float freq) override
    {
        const double v = freq;
        chk_runtime(mi355_costas_set_state(d_h, nullptr, &v), "mi355_costas_set_state");
    }
    void set_phase(float phase) override
    {
        const double v = phase;
        chk_runtime(mi355_costas_set_state(d_h, &v, nullptr), "mi355_costas_set_state");
    }
    int work(int noutput_items, gr_vector_const_void_star &input_items, gr_vector_void_star &output_items) override
    {
        float *foptr = output_items.size() >= 2 ? (float *)output_items[1] : nullptr;  // :456-458
        chk_runtime(mi355_costas_work(d_h, (size_t)noutput_items, input_items[0], output_items[0], foptr), "mi355_costas_work");
        return noutput_items;
    }
};

}  // namespace

clCostasLoop::sptr clCostasLoop::make(int openCLPlatformType, int devSelector, int platformId, int devId, float loop_bw, int order,
                                      int setDebug)
{
    return sched::adopt(new clCostasLoop_impl(openCLPlatformType, devSelector, platformId, devId, loop_bw, order, setDebug != 0));
}

}  // namespace clenabled
}  // namespace gr
