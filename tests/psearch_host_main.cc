// Stand-alone program around host/lib/clPulseSearch_impl.cc for tests/test_psearch_host.py: the block class over a STUB of the C ABI,
// no device.  The stub's mi355_psearch_work reads every input float the contract names ((n + Hs) R D) and writes every peak record
// (n / Tb x R D) -- the test hands it heap buffers of exactly that size, so under -fsanitize=address,undefined a work() that passes a
// sample too few or the wrong count is caught -- and records what it was handed.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <vector>

struct mi355_psearch {
    int R, D, K, Tb, order, generic;
    long long calls, last_n, last_pitch;
    std::vector<float> mean, isg;
};

static int stub_plan(int R, int D, int K, int Tb, int order, long long *fi, long long *hi, long long *pb)
{
    if (R < 1 || R > 4096 || D < 1 || D > 4096 || K < 1 || K > 13 || Tb < 16 || Tb > (1 << 24) - 1 || (order != 0 && order != 1)) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (fi) *fi = (long long)R * D;
    if (hi) *hi = (1ll << (K - 1)) - 1;
    if (pb) *pb = (long long)R * D;
    return MI355_OK;
}

extern "C" {
int mi355_psearch_plan(int R, int D, int K, int Tb, int order, long long *fi, long long *hi, long long *pb) { return stub_plan(R, D, K, Tb, order, fi, hi, pb); }
int mi355_psearch_create(mi355_ctx *ctx, int R, int D, int K, int Tb, int order, const float *mean, const float *isg, mi355_psearch **out)
{
    if (!ctx || !out || stub_plan(R, D, K, Tb, order, nullptr, nullptr, nullptr)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    const size_t S = (size_t)R * D;
    *out = new mi355_psearch{R, D, K, Tb, order, 0, 0, 0, -1, mean ? std::vector<float>(mean, mean + S) : std::vector<float>(S, 0.0f),
                             isg ? std::vector<float>(isg, isg + S) : std::vector<float>(S, 1.0f)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_psearch_destroy(mi355_psearch *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_psearch_set_stats(mi355_psearch *h, const float *mean, const float *isg)
{
    if (!mean || !isg) { g_err = "invalid argument: stub stats"; return MI355_ERR_INVALID_ARG; }
    h->mean.assign(mean, mean + h->mean.size());
    h->isg.assign(isg, isg + h->isg.size());
    return MI355_OK;
}
int mi355_psearch_get_stats(const mi355_psearch *h, float *mean, float *isg, long long cap)
{
    if (cap < (long long)h->mean.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(mean, h->mean.data(), h->mean.size() * 4);
    memcpy(isg, h->isg.data(), h->isg.size() * 4);
    return MI355_OK;
}
int mi355_psearch_set_generic(mi355_psearch *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_psearch_route(const mi355_psearch *h) { return h->generic ? "generic stub" : "tiled stub"; }
int mi355_psearch_work(mi355_psearch *h, long long n, const void *in, long long in_pitch, void *peaks, void *cands, long long max_cands, void *counts)
{
    if (n % h->Tb || cands || counts || max_cands) { g_err = "invalid argument: stub work"; return MI355_ERR_INVALID_ARG; }
    const long long S = (long long)h->R * h->D, Hs = (1ll << (h->K - 1)) - 1;
    const float *x = (const float *)in;
    float sum = 0.f;
    for (long long i = 0; i < (n + Hs) * S; i++) sum += x[i];  // every float the contract reads
    auto *y = (gr::clenabled::clPulseSearch::peak *)peaks;
    for (long long i = 0; i < n / h->Tb * S; i++) y[i] = {(float)(h->calls + 1) + 0.f * sum, (uint32_t)i};
    h->calls++;
    h->last_n = n;
    h->last_pitch = in_pitch;
    return MI355_OK;
}
}

using gr::clenabled::clPulseSearch;

// one work() call on exact-size heap buffers, as the scheduler makes it: n decimation + history() - 1 input items; returns what
// work() returned, or -1 when a record of the output is not the stub's
static int call(clPulseSearch &ps, int n, int call_no)
{
    const size_t in_bytes = ((size_t)n * ps.decimation() + ps.history() - 1) * (size_t)ps.input_signature()->sizeof_stream_item(0);
    const size_t out_bytes = (size_t)n * (size_t)ps.output_signature()->sizeof_stream_item(0);
    std::vector<float> x(in_bytes / 4, 1.0f);
    std::vector<clPulseSearch::peak> y(out_bytes / sizeof(clPulseSearch::peak), clPulseSearch::peak{-7.0f, 0xABCDu});
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    const int got = ps.work(n, in, out);
    for (size_t i = 0; i < y.size(); i++)
        if (y[i].snr != (float)call_no || y[i].loc != (uint32_t)i) return -1;
    return got;
}

static int run(int R, int D, int K, int Tb)
{
    const size_t S = (size_t)R * D;
    const int Hs = (1 << (K - 1)) - 1;
    std::vector<float> m(S), g(S);
    for (size_t i = 0; i < S; i++) { m[i] = (float)i; g[i] = 1.0f / (float)(i + 1); }
    auto ps = clPulseSearch::make(1, 2, 0, 0, R, D, K, Tb, m, g);
    // io signature, item sizes, decimation, history
    CHECK(ps->input_signature()->min_streams() == 1 && ps->input_signature()->max_streams() == 1);
    CHECK(ps->output_signature()->min_streams() == 1 && ps->output_signature()->max_streams() == 1);
    CHECK(ps->input_signature()->sizeof_stream_item(0) == 4 * R * D && ps->output_signature()->sizeof_stream_item(0) == 8 * R * D);
    CHECK(sizeof(clPulseSearch::peak) == 8);
    CHECK((int)ps->history() == Hs + 1 && ps->lookahead() == Hs && (int)ps->decimation() == Tb);
    CHECK(ps->route() == "tiled stub" && ps->mean() == m && ps->inv_sigma() == g);
    // what work() hands the library: n Tb outputs, n Tb + Hs samples behind the pointer, TIME_MAJOR with in_pitch 0, no candidates
    int calls = 0;
    for (int n : {1, 2, 5}) CHECK(call(*ps, n, ++calls) == n);
    ps->set_generic(true);
    CHECK(ps->route() == "generic stub");
    // set_stats: the sizes are checked by the block; a refused update keeps the old values
    std::vector<float> m2(S, 2.0f), g2(S, 0.25f);
    ps->set_stats(m2, g2);
    CHECK(ps->mean() == m2 && ps->inv_sigma() == g2);
    for (size_t bad : {(size_t)0, S - 1, S + 1, 2 * S}) {
        CHECK(throws<std::invalid_argument>([&] { ps->set_stats(std::vector<float>(bad, 0.f), g2); }) && ps->mean() == m2 && ps->inv_sigma() == g2);
        CHECK(throws<std::invalid_argument>([&] { ps->set_stats(m2, std::vector<float>(bad, 0.f)); }) && ps->mean() == m2 && ps->inv_sigma() == g2);
    }
    CHECK(call(*ps, 3, ++calls) == 3);
    // no statistics at make(): mean 0, inv_sigma 1
    auto z = clPulseSearch::make(1, 2, 0, 0, R, D, K, Tb);
    CHECK(z->mean() == std::vector<float>(S, 0.0f) && z->inv_sigma() == std::vector<float>(S, 1.0f));
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 1, 1, 16}, {2, 5, 4, 32}, {3, 17, 9, 48}, {4, 7, 13, 16}, {64, 3, 2, 100}}) {
        const int rc = run(s[0], s[1], s[2], s[3]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{0, 8, 4, 16}, {4097, 8, 4, 16}, {2, 0, 4, 16}, {2, 4097, 4, 16}, {2, 8, 0, 16}, {2, 8, 14, 16}, {2, 8, 4, 15},
                                               {2, 8, 4, 1 << 24}};
    for (const auto &s : bad) CHECK(throws<std::invalid_argument>([&] { clPulseSearch::make(1, 2, 0, 99, s[0], s[1], s[2], s[3]); }));
    // statistics of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([] { clPulseSearch::make(1, 2, 0, 99, 2, 8, 4, 16, std::vector<float>(7, 0.f)); }));
    CHECK(throws<std::runtime_error>([] { clPulseSearch::make(1, 2, 0, 99, 2, 8, 4, 16); }, "no such device") && g_live_ctx == 0);
    printf("psearch host ok\n");
    return 0;
}
