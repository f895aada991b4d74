// clSignalSource_impl: the reference's lib/clSignalSource_impl.cc over the C ABI (mi355_sigsource_*).  The phase accumulator is the
// handle's; work() produces noutput_items items and advances it (:329-415).
#include <clenabled/clenabled.h>
#include <mi355_clenabled.h>

#include <stdexcept>
#include <string>

namespace gr {
namespace clenabled {
namespace {

void chk(int rc, const char *what)
{
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + mi355_strerror(rc) + ": " + mi355_last_error());
}

int item_bytes(int idataType) { return idataType == DTYPE_COMPLEX ? (int)sizeof(gr_complex) : 4; }  // :46-62

class clSignalSource_impl : public clSignalSource {
    mi355_ctx *d_ctx = nullptr;
    mi355_sigsource *d_h = nullptr;

public:
    clSignalSource_impl(int idataType, int openCLPlatformType, int devSelector, int platformId, int devId, double samp_rate, int waveform,
                        double freq, float amplitude, bool setDebug)
        : gr::sync_block("clSignalSource", gr::io_signature::make(0, 0, 0), gr::io_signature::make(1, 1, item_bytes(idataType)))  // :66-69
    {
        chk(mi355_ctx_create(openCLPlatformType, devSelector, platformId, devId, setDebug ? 1 : 0, &d_ctx), "mi355_ctx_create");
        const int rc = mi355_sigsource_create(d_ctx, idataType, samp_rate, waveform, freq, amplitude, &d_h);
        if (rc) {
            const std::string msg = std::string("mi355_sigsource_create: ") + mi355_strerror(rc) + ": " + mi355_last_error();
            mi355_ctx_destroy(d_ctx);
            if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(msg);
            throw std::runtime_error(msg);
        }
    }
    ~clSignalSource_impl() override
    {
        mi355_sigsource_destroy(d_h);
        mi355_ctx_destroy(d_ctx);
    }
    void set_frequency(double frequency) override { chk(mi355_sigsource_set_frequency(d_h, frequency), "mi355_sigsource_set_frequency"); }
    void set_phase(double angle_pos) override { chk(mi355_sigsource_set_phase(d_h, angle_pos), "mi355_sigsource_set_phase"); }
    double get_angle_pos() const override
    {
        double v = 0;
        chk(mi355_sigsource_get_state(d_h, &v, nullptr), "mi355_sigsource_get_state");
        return v;
    }
    double get_angle_rate() const override
    {
        double v = 0;
        chk(mi355_sigsource_get_state(d_h, nullptr, &v), "mi355_sigsource_get_state");
        return v;
    }
    int work(int noutput_items, gr_vector_const_void_star &, gr_vector_void_star &output_items) override
    {
        chk(mi355_sigsource_work(d_h, (size_t)noutput_items, output_items[0]), "mi355_sigsource_work");
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
