// Stand-alone program around host/lib/clFilterbankCleaner_impl.cc for tests/test_fbclean_host.py: the block class over a STUB of the C
// ABI, no device.  The stub's mi355_fbclean_work reads every input float the contract names (n R F) and writes every output it is
// handed (n R F floats, n / Tb x R F channel flags, n R time flags) -- the test hands the block heap buffers of exactly the scheduler's
// sizes, so under -fsanitize=address,undefined a work() that passes a wrong count or a short buffer is caught -- and records what it
// was handed.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <cmath>
#include <vector>

struct mi355_fbclean {
    int R, F, Tb, generic;
    double nd, lo, hi, td;
    int zero_dm;
    long long calls, last_n;
    bool had_cflags, had_tflags, had_stats;
    std::vector<uint8_t> mask;
};

static int stub_plan(int R, int F, int Tb, long long *a, long long *b, long long *c)
{
    if (R < 1 || R > 4096 || F < 1 || F > 16384 || Tb < 16 || Tb > 4096 || Tb % 16) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (a) *a = (long long)R * F;
    if (b) *b = (long long)R * F;
    if (c) *c = R;
    return MI355_OK;
}

static bool stub_limits_ok(double nd, double lo, double hi, double td, int z) { return std::isfinite(nd) && nd > 0 && lo <= hi && td >= 0 && (z == 0 || z == 1); }

extern "C" {
int mi355_fbclean_plan(int R, int F, int Tb, long long *a, long long *b, long long *c) { return stub_plan(R, F, Tb, a, b, c); }
int mi355_fbclean_create(mi355_ctx *ctx, int R, int F, int Tb, double nd, double lo, double hi, double td, int z, const uint8_t *mask, mi355_fbclean **out)
{
    if (!ctx || !out || stub_plan(R, F, Tb, nullptr, nullptr, nullptr) || !stub_limits_ok(nd, lo, hi, td, z)) {
        g_err = "invalid argument: stub create";
        return MI355_ERR_INVALID_ARG;
    }
    *out = new mi355_fbclean{R, F, Tb, 0, nd, lo, hi, td, z, 0, 0, false, false, false,
                             mask ? std::vector<uint8_t>(mask, mask + F) : std::vector<uint8_t>((size_t)F, 0)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_fbclean_destroy(mi355_fbclean *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_fbclean_set_limits(mi355_fbclean *h, double nd, double lo, double hi, double td, int z)
{
    if (!stub_limits_ok(nd, lo, hi, td, z)) { g_err = "invalid argument: stub limits"; return MI355_ERR_INVALID_ARG; }
    h->nd = nd; h->lo = lo; h->hi = hi; h->td = td; h->zero_dm = z;
    return MI355_OK;
}
int mi355_fbclean_get_limits(const mi355_fbclean *h, double *nd, double *lo, double *hi, double *td, int *z)
{
    *nd = h->nd; *lo = h->lo; *hi = h->hi; *td = h->td; *z = h->zero_dm;
    return MI355_OK;
}
int mi355_fbclean_set_mask(mi355_fbclean *h, const uint8_t *mask)
{
    if (!mask) { g_err = "invalid argument: stub mask"; return MI355_ERR_INVALID_ARG; }
    h->mask.assign(mask, mask + h->F);
    return MI355_OK;
}
int mi355_fbclean_get_mask(const mi355_fbclean *h, uint8_t *out, long long cap)
{
    if (cap < (long long)h->mask.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(out, h->mask.data(), h->mask.size());
    return MI355_OK;
}
int mi355_fbclean_set_generic(mi355_fbclean *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_fbclean_route(const mi355_fbclean *h) { return h->generic ? "generic stub" : "slab stub"; }
int mi355_fbclean_work(mi355_fbclean *h, long long n, const void *in, void *out, void *cflags, void *tflags, void *stats)
{
    if (n <= 0 || n % h->Tb || !in || !out) { g_err = "invalid argument: stub work"; return MI355_ERR_INVALID_ARG; }
    const long long RF = (long long)h->R * h->F, nb = n / h->Tb;
    const float *x = (const float *)in;
    float *y = (float *)out;
    for (long long i = 0; i < n * RF; i++) y[i] = x[i] + (float)(h->calls + 1);  // every float the contract reads and writes
    if (cflags)
        for (long long i = 0; i < nb * RF; i++) ((uint8_t *)cflags)[i] = (uint8_t)((i / RF) + 1);  // the block's number within the call, plus one
    if (tflags)
        for (long long i = 0; i < n * h->R; i++) ((uint8_t *)tflags)[i] = (uint8_t)(i % 251);
    h->calls++;
    h->last_n = n;
    h->had_cflags = cflags != nullptr;
    h->had_tflags = tflags != nullptr;
    h->had_stats = stats != nullptr;
    return MI355_OK;
}
}

using gr::clenabled::clFilterbankCleaner;

// one work() call on exact-size heap buffers, as the scheduler makes it, with `nout` output streams; returns what work() returned, or
// -1 when an output is not the stub's
static int call(clFilterbankCleaner &fc, int n, int nout, int call_no, int Tb)
{
    const size_t isz = (size_t)fc.input_signature()->sizeof_stream_item(0);
    std::vector<float> x((size_t)n * isz / 4, 1.0f), y((size_t)n * (size_t)fc.output_signature()->sizeof_stream_item(0) / 4, -7.0f);
    std::vector<uint8_t> tf((size_t)n * (size_t)fc.output_signature()->sizeof_stream_item(1), 0xEE);
    std::vector<uint8_t> cf((size_t)n * (size_t)fc.output_signature()->sizeof_stream_item(2), 0xEE);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    if (nout >= 2) out.push_back(tf.data());
    if (nout >= 3) out.push_back(cf.data());
    const int got = fc.work(n, in, out);
    const int whole = n - n % Tb;
    for (size_t i = 0; i < y.size(); i++)
        if (y[i] != (i < (size_t)whole * isz / 4 ? 1.0f + (float)call_no : -7.0f)) return -1;
    const size_t R = (size_t)fc.output_signature()->sizeof_stream_item(1), RF = (size_t)fc.output_signature()->sizeof_stream_item(2);
    for (size_t i = 0; i < tf.size(); i++)
        if (tf[i] != (nout >= 2 && i < (size_t)whole * R ? (uint8_t)(i % 251) : 0xEE)) return -1;
    for (size_t i = 0; i < cf.size(); i++)  // item t carries the flags of block t / Tb
        if (cf[i] != (nout >= 3 && i < (size_t)whole * RF ? (uint8_t)(i / RF / (size_t)Tb + 1) : 0xEE)) return -1;
    return got;
}

static int run(int R, int F, int Tb)
{
    std::vector<uint8_t> mask((size_t)F, 0);
    mask[(size_t)F / 2] = 1;
    auto fc = clFilterbankCleaner::make(1, 2, 0, 0, R, F, Tb, 16.0, 0.5, 1.5, 5.0, true, mask);
    // io signature, item sizes, output multiple, history
    CHECK(fc->input_signature()->min_streams() == 1 && fc->input_signature()->max_streams() == 1);
    CHECK(fc->output_signature()->min_streams() == 1 && fc->output_signature()->max_streams() == 3);
    CHECK(fc->input_signature()->sizeof_stream_item(0) == 4 * R * F && fc->output_signature()->sizeof_stream_item(0) == 4 * R * F);
    CHECK(fc->output_signature()->sizeof_stream_item(1) == R && fc->output_signature()->sizeof_stream_item(2) == R * F);
    CHECK((int)fc->history() == 1 && fc->output_multiple() == Tb && fc->block_len() == Tb);
    CHECK(fc->route() == "slab stub" && fc->mask() == mask && fc->limits() == (std::vector<double>{16.0, 0.5, 1.5, 5.0, 1.0}));
    // what work() hands the library: whole blocks, the optional outputs only when the stream is connected
    int calls = 0;
    for (int nout : {1, 2, 3})
        for (int nb : {1, 3}) CHECK(call(*fc, nb * Tb, nout, ++calls, Tb) == nb * Tb);
    CHECK(call(*fc, 2 * Tb + 5, 3, ++calls, Tb) == 2 * Tb);  // a ragged offer: whole blocks only, nothing behind them is touched
    CHECK(call(*fc, Tb - 1, 3, calls, Tb) == 0);            // less than a block: nothing is done
    fc->set_generic(true);
    CHECK(fc->route() == "generic stub");
    // set_limits: a refused update keeps the old values
    fc->set_limits(8.0, 0.25, 2.0, 3.0, false);
    CHECK(fc->limits() == (std::vector<double>{8.0, 0.25, 2.0, 3.0, 0.0}));
    CHECK(throws<std::invalid_argument>([&] { fc->set_limits(0.0, 0.25, 2.0, 3.0, false); }));
    CHECK(fc->limits() == (std::vector<double>{8.0, 0.25, 2.0, 3.0, 0.0}));
    // set_mask: the size is checked by the block
    std::vector<uint8_t> m2((size_t)F, 1);
    fc->set_mask(m2);
    CHECK(fc->mask() == m2);
    for (size_t bad : {(size_t)0, (size_t)F - 1, (size_t)F + 1})
        CHECK(throws<std::invalid_argument>([&] { fc->set_mask(std::vector<uint8_t>(bad, 0)); }) && fc->mask() == m2);
    // no mask and no limits at make(): nothing masked, every test disabled
    auto z = clFilterbankCleaner::make(1, 2, 0, 0, R, F, Tb);
    CHECK(z->mask() == std::vector<uint8_t>((size_t)F, 0));
    const std::vector<double> lim = z->limits();
    CHECK(lim[0] == 1.0 && lim[1] == -INFINITY && lim[2] == INFINITY && lim[3] == INFINITY && lim[4] == 0.0);
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 1, 16}, {2, 5, 32}, {3, 52, 48}, {2, 256, 64}}) {
        const int rc = run(s[0], s[1], s[2]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{0, 8, 16}, {4097, 8, 16}, {2, 0, 16}, {2, 16385, 16}, {2, 8, 0}, {2, 8, 24}, {2, 8, 4112}};
    for (const auto &s : bad) CHECK(throws<std::invalid_argument>([&] { clFilterbankCleaner::make(1, 2, 0, 99, s[0], s[1], s[2]); }));
    // a mask of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([] { clFilterbankCleaner::make(1, 2, 0, 99, 2, 8, 16, 1.0, 0.0, 2.0, 1.0, false, std::vector<uint8_t>(7, 0)); }));
    CHECK(throws<std::runtime_error>([] { clFilterbankCleaner::make(1, 2, 0, 99, 2, 8, 16); }, "no such device") && g_live_ctx == 0);
    // a refused create gives the context back
    CHECK(throws<std::invalid_argument>([] { clFilterbankCleaner::make(1, 2, 0, 0, 2, 8, 16, -1.0); }) && g_live_ctx == 0 && g_live_handles == 0);
    printf("fbclean host ok\n");
    return 0;
}
