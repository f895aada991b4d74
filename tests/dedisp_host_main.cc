// Stand-alone program around host/lib/clDedisperser_impl.cc for tests/test_dedisp_host.py: the block class over a STUB of the C ABI,
// no device.  The stub's mi355_dedisp_work reads every input float the contract names ((n + max_delay) R F) and writes every output
// float (n R D) -- the test hands it heap buffers of exactly that size, so under -fsanitize=address,undefined a work() that passes a
// sample too few or the wrong count is caught -- and records what it was handed.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <vector>

struct mi355_dedisp {
    int R, F, D, H, order, generic;
    long long calls, last_n, last_pitch;
    std::vector<int32_t> tab;
};

static int stub_plan(int R, int F, int D, int H, int order, long long *fi, long long *hi, long long *fo)
{
    if (R < 1 || R > 4096 || F < 1 || F > 16384 || D < 1 || D > 4096 || H < 0 || H > (1 << 20) || (order != 0 && order != 1)) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (fi) *fi = (long long)R * F;
    if (hi) *hi = H;
    if (fo) *fo = (long long)R * D;
    return MI355_OK;
}

static bool stub_table_ok(const int32_t *t, size_t n, int H)
{
    for (size_t i = 0; i < n; i++)
        if (t[i] < -1 || t[i] > H) { g_err = "invalid argument: stub delay"; return false; }
    return true;
}

extern "C" {
int mi355_dedisp_plan(int R, int F, int D, int H, int order, long long *fi, long long *hi, long long *fo) { return stub_plan(R, F, D, H, order, fi, hi, fo); }
int mi355_dedisp_create(mi355_ctx *ctx, int R, int F, int D, int H, int order, const int32_t *delays, mi355_dedisp **out)
{
    if (!ctx || !out || stub_plan(R, F, D, H, order, nullptr, nullptr, nullptr)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    const size_t n = (size_t)D * F;
    if (delays && !stub_table_ok(delays, n, H)) return MI355_ERR_INVALID_ARG;
    *out = new mi355_dedisp{R, F, D, H, order, 0, 0, 0, -1, delays ? std::vector<int32_t>(delays, delays + n) : std::vector<int32_t>(n, 0)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_dedisp_destroy(mi355_dedisp *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_dedisp_set_delays(mi355_dedisp *h, const int32_t *delays)
{
    if (!stub_table_ok(delays, h->tab.size(), h->H)) return MI355_ERR_INVALID_ARG;
    h->tab.assign(delays, delays + h->tab.size());
    return MI355_OK;
}
int mi355_dedisp_get_delays(const mi355_dedisp *h, int32_t *out, long long cap)
{
    if (cap < (long long)h->tab.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(out, h->tab.data(), h->tab.size() * 4);
    return MI355_OK;
}
int mi355_dedisp_set_generic(mi355_dedisp *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_dedisp_route(const mi355_dedisp *h) { return h->generic ? "generic stub" : "tiled stub"; }
int mi355_dedisp_work(mi355_dedisp *h, long long n, const void *in, void *out, long long out_pitch)
{
    const float *x = (const float *)in;
    float sum = 0.f;
    for (long long i = 0; i < (n + h->H) * h->R * h->F; i++) sum += x[i];  // every float the contract reads
    float *y = (float *)out;
    for (long long i = 0; i < n * h->R * h->D; i++) y[i] = (float)(h->calls + 1) + 0.f * sum;
    h->calls++;
    h->last_n = n;
    h->last_pitch = out_pitch;
    return MI355_OK;
}
}

using gr::clenabled::clDedisperser;

// one work() call on exact-size heap buffers, as the scheduler makes it: n + history() - 1 input items; returns what work() returned,
// or -1 when a float of the output is not the stub's
static int call(clDedisperser &dd, int n, int call_no)
{
    const size_t in_bytes = (size_t)(n + dd.history() - 1) * (size_t)dd.input_signature()->sizeof_stream_item(0);
    const size_t out_bytes = (size_t)n * (size_t)dd.output_signature()->sizeof_stream_item(0);
    std::vector<float> x(in_bytes / 4, 1.0f);
    std::vector<float> y(out_bytes / 4, -7.0f);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    const int got = dd.work(n, in, out);
    for (float v : y)
        if (v != (float)call_no) return -1;
    return got;
}

static int run(int R, int F, int D, int H)
{
    const size_t nt = (size_t)D * F;
    std::vector<int32_t> t(nt);
    for (size_t i = 0; i < nt; i++) t[i] = (int32_t)(i % (size_t)(H + 2)) - 1;  // -1 .. H
    auto dd = clDedisperser::make(1, 2, 0, 0, R, F, D, H, t);
    // io signature, item sizes, history
    CHECK(dd->input_signature()->min_streams() == 1 && dd->input_signature()->max_streams() == 1);
    CHECK(dd->output_signature()->min_streams() == 1 && dd->output_signature()->max_streams() == 1);
    CHECK(dd->input_signature()->sizeof_stream_item(0) == 4 * R * F && dd->output_signature()->sizeof_stream_item(0) == 4 * R * D);
    CHECK((int)dd->history() == H + 1 && dd->max_delay() == H);
    CHECK(dd->route() == "tiled stub" && dd->delays() == t);
    // what work() hands the library: n outputs, n + H samples behind the pointer, TIME_MAJOR with out_pitch 0
    int calls = 0;
    for (int n : {1, 2, 7, 33}) CHECK(call(*dd, n, ++calls) == n);
    dd->set_generic(true);
    CHECK(dd->route() == "generic stub");
    // set_delays: the size is checked by the block, the values by the library; a refused update keeps the old table
    std::vector<int32_t> t2(nt, H);
    dd->set_delays(t2);
    CHECK(dd->delays() == t2);
    for (size_t bad : {(size_t)0, nt - 1, nt + 1, 2 * nt})
        CHECK(throws<std::invalid_argument>([&] { dd->set_delays(std::vector<int32_t>(bad, 0)); }) && dd->delays() == t2);
    for (int32_t v : {-2, H + 1}) {
        std::vector<int32_t> t3(nt, 0);
        t3[nt / 2] = v;
        CHECK(throws<std::invalid_argument>([&] { dd->set_delays(t3); }) && dd->delays() == t2);
    }
    CHECK(call(*dd, 5, ++calls) == 5);
    // no table at make(): all zero
    auto z = clDedisperser::make(1, 2, 0, 0, R, F, D, H);
    CHECK(z->delays() == std::vector<int32_t>(nt, 0));
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 1, 1, 0}, {2, 20, 5, 19}, {3, 80, 40, 200}, {4, 7, 17, 1}, {64, 16, 3, 50}}) {
        const int rc = run(s[0], s[1], s[2], s[3]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{0, 8, 4, 5}, {4097, 8, 4, 5}, {2, 0, 4, 5}, {2, 16385, 4, 5}, {2, 8, 0, 5}, {2, 8, 4097, 5}, {2, 8, 4, -1},
                                               {2, 8, 4, (1 << 20) + 1}};
    for (const auto &s : bad) CHECK(throws<std::invalid_argument>([&] { clDedisperser::make(1, 2, 0, 99, s[0], s[1], s[2], s[3]); }));
    // a table of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([] { clDedisperser::make(1, 2, 0, 99, 2, 8, 4, 5, std::vector<int32_t>(7, 0)); }));
    // refused by the library: the context is given back
    CHECK(throws<std::invalid_argument>([] { clDedisperser::make(1, 2, 0, 0, 2, 8, 4, 5, std::vector<int32_t>(32, 6)); }) && g_live_ctx == 0);
    CHECK(throws<std::runtime_error>([] { clDedisperser::make(1, 2, 0, 99, 2, 8, 4, 5); }, "no such device"));
    printf("dedisp host ok\n");
    return 0;
}
