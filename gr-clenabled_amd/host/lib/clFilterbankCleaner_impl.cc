// clFilterbankCleaner_impl: exact RFI excision over the C ABI (mi355_fbclean_*).  A sync_block whose item is one time sample of R F
// floats and whose output multiple is block_len, so every work() call hands the library whole blocks.  Output 0 is the cleaned
// filterbank; the optional output 1 carries the R time-sample flags of each item and the optional output 2 the R F channel flags of
// the block the item lies in (the same bytes for all block_len items of a block, so that the stream stays sample-synchronous).  The
// limits and the mask live in the library handle; the block keeps no stream state.
#include <clenabled/clenabled.h>
#include "block_base.h"

#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {
namespace {

struct Plan {
    long long floats = 0, cflag_bytes = 0, tflag_bytes = 0;
};

// argument errors before any device work (and before the io signatures, which need the sizes)
Plan plan(int R, int F, int Tb)
{
    Plan p;
    chk_arg(mi355_fbclean_plan(R, F, Tb, &p.floats, &p.cflag_bytes, &p.tflag_bytes), "clFilterbankCleaner");
    check_stream_item("clFilterbankCleaner", {p.floats * 4});
    return p;
}

class clFilterbankCleaner_impl : public clFilterbankCleaner, BlockBase<mi355_fbclean, mi355_fbclean_destroy> {
    const Plan d_plan;
    const size_t d_channels;
    const int d_block_len;
    std::vector<uint8_t> d_cflags;  // [block][R][F] of one work() call
    std::mutex d_lock;

public:
    clFilterbankCleaner_impl(int openCLPlatformType, int devSelector, int platformId, int devId, int R, int F, int Tb, double nd, double sk_lo,
                             double sk_hi, double td, bool zero_dm, const std::vector<uint8_t> &mask, bool setDebug, const Plan &p)
        : gr::sync_block("clFilterbankCleaner", gr::io_signature::make(1, 1, (int)(p.floats * 4)),
                         gr::io_signature::makev(1, 3, std::vector<int>{(int)(p.floats * 4), (int)p.tflag_bytes, (int)p.cflag_bytes})),
          d_plan(p), d_channels((size_t)F), d_block_len(Tb)
    {
        if (!mask.empty() && mask.size() != d_channels)
            throw std::invalid_argument("clFilterbankCleaner: the mask holds " + std::to_string(mask.size()) + " entries, the geometry has " +
                                        std::to_string(d_channels) + " channels");
        set_output_multiple(Tb);
        d_ctx.open(openCLPlatformType, devSelector, platformId, devId, setDebug, chk_arg);
        created(mi355_fbclean_create(d_ctx, R, F, Tb, nd, sk_lo, sk_hi, td, zero_dm ? 1 : 0, mask.empty() ? nullptr : mask.data(), d_h.adopt()),
                "mi355_fbclean_create");
    }
    void set_limits(double nd, double sk_lo, double sk_hi, double td, bool zero_dm) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fbclean_set_limits(d_h, nd, sk_lo, sk_hi, td, zero_dm ? 1 : 0), "mi355_fbclean_set_limits");
    }
    std::vector<double> limits() const override
    {
        std::vector<double> v(5);
        int z = 0;
        chk_arg(mi355_fbclean_get_limits(d_h, &v[0], &v[1], &v[2], &v[3], &z), "mi355_fbclean_get_limits");
        v[4] = z;
        return v;
    }
    void set_mask(const std::vector<uint8_t> &mask) override
    {
        if (mask.size() != d_channels)
            throw std::invalid_argument("clFilterbankCleaner: set_mask() takes " + std::to_string(d_channels) + " entries, got " +
                                        std::to_string(mask.size()));
        std::lock_guard<std::mutex> g(d_lock);
        chk_arg(mi355_fbclean_set_mask(d_h, mask.data()), "mi355_fbclean_set_mask");
    }
    std::vector<uint8_t> mask() const override
    {
        std::vector<uint8_t> t(d_channels);
        chk_arg(mi355_fbclean_get_mask(d_h, t.data(), (long long)t.size()), "mi355_fbclean_get_mask");
        return t;
    }
    int block_len() const override { return d_block_len; }
    void set_generic(bool on) override { chk_arg(mi355_fbclean_set_generic(d_h, on ? 1 : 0), "mi355_fbclean_set_generic"); }
    std::string route() const override { return mi355_fbclean_route(d_h); }
    int work(int noutput_items, gr_vector_const_void_star &in, gr_vector_void_star &out) override
    {
        std::lock_guard<std::mutex> g(d_lock);
        const int n = noutput_items - noutput_items % d_block_len;  // whole blocks (the scheduler keeps to the output multiple)
        if (n == 0) return 0;
        void *tflags = out.size() >= 2 ? out[1] : nullptr;
        uint8_t *per_item = out.size() >= 3 ? (uint8_t *)out[2] : nullptr;
        const size_t cb = (size_t)d_plan.cflag_bytes, nblk = (size_t)(n / d_block_len);
        if (per_item) d_cflags.resize(nblk * cb);
        chk_arg(mi355_fbclean_work(d_h, n, in[0], out[0], per_item ? d_cflags.data() : nullptr, tflags, nullptr), "mi355_fbclean_work");
        if (per_item)
            for (size_t t = 0; t < (size_t)n; t++) memcpy(per_item + t * cb, d_cflags.data() + (t / (size_t)d_block_len) * cb, cb);
        return n;
    }
};

}  // namespace

clFilterbankCleaner::sptr clFilterbankCleaner::make(int openCLPlatformType, int devSelector, int platformId, int devId, int num_rows, int num_channels,
                                                    int block_len, double nd, double sk_lo, double sk_hi, double td, bool zero_dm,
                                                    const std::vector<uint8_t> &mask, int setDebug)
{
    const Plan p = plan(num_rows, num_channels, block_len);
    return sched::adopt(new clFilterbankCleaner_impl(openCLPlatformType, devSelector, platformId, devId, num_rows, num_channels, block_len, nd, sk_lo,
                                                     sk_hi, td, zero_dm, mask, setDebug != 0, p));
}

}  // namespace clenabled
}  // namespace gr
