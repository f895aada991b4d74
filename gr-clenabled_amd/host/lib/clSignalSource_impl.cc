// clSignalSource_impl: the reference's lib/clSignalSource_impl.cc over the C ABI (mi355_sigsource_*).  The phase accumulator is the
// handle's; work() produces noutput_items items and advances it (:329-415).
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <stdexcept>
#include <string>

namespace gr {
namespace clenabled {
namespace {

int item_bytes(int idataType) { return idataType == DTYPE_COMPLEX ? (int)sizeof(gr_complex) : 4; }  // :46-62

class clSignalSource_impl : public clSignalSource, BlockBase<mi355_sigsource, mi355_sigsource_destroy> {
public:
    clSignalSource_impl(int idataType, int openCLPlatformType, int devSelector, int platformId, int devId, double samp_rate, int waveform,
                        double freq, float amplitude, bool setDebug)
        : gr::sync_block("clSignalSource", gr::io_signature::make(0, 0, 0), gr::io_signature::make(1, 1, item_bytes(idataType)))  // :66-69
    {
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug);
        created(mi355_sigsource_create(d_ctx, idataType, samp_rate, waveform, freq, amplitude, d_h.adopt()), "mi355_sigsource_create");
    }
    void set_frequency(double frequency) override { chk_runtime(mi355_sigsource_set_frequency(d_h, frequency), "mi355_sigsource_set_frequency"); }
    void set_phase(double angle_pos) override { chk_runtime(mi355_sigsource_set_phase(d_h, angle_pos), "mi355_sigsource_set_phase"); }
    double get_angle_pos() const override
    {
        double v = 0;
        chk_runtime(mi355_sigsource_get_state(d_h, &v, nullptr), "mi355_sigsource_get_state");
        return v;
    }
    double get_angle_rate() const override
    {
        double v = 0;
        chk_runtime(mi355_sigsource_get_state(d_h, nullptr, &v), "mi355_sigsource_get_state");
        return v;
    }
    int work(int noutput_items, gr_vector_const_void_star &, gr_vector_void_star &output_items) override
    {
        chk_runtime(mi355_sigsource_work(d_h, (size_t)noutput_items, output_items[0]), "mi355_sigsource_work");
        return noutput_items;
    }
};

}  // namespace

clSignalSource::sptr clSignalSource::make(int idataType, int openCLPlatformType, int devSelector, int platformId, int devId, double samp_rate,
                                          int waveform, double freq, float amplitude, int setDebug)
{
    return sched::adopt(new clSignalSource_impl(idataType, openCLPlatformType, devSelector, platformId, devId, samp_rate, waveform, freq,
                                                amplitude, setDebug != 0));
}

}  // namespace clenabled
}  // namespace gr
