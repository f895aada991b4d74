// Stand-alone program around host/lib/clPeriodSearch_impl.cc for tests/test_ffa_host.py: the block class over a STUB of the C ABI, no
// device.  The stub's mi355_ffa_work reads every input float the contract names (S series of N = 2^L p_hi floats at in_pitch) and
// writes every peak record (S P 2^L) and, if asked, every profile float a call may write (j < p of S P 2^L rows of pitch p_hi) -- the
// test hands it heap buffers of exactly the item sizes, so under -fsanitize=address,undefined a work() that passes a wrong pointer, a
// wrong pitch or a wrong item offset is caught -- and records what it was handed.  The stub's plan, shift and period are the
// contract's arithmetic, written out again here.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <cmath>
#include <vector>

struct mi355_ffa {
    int S, p_lo, p_hi, L, K, generic;
    long long calls, last_pitch;
    bool last_profiles;
    std::vector<float> mean, isg;
};

static int stub_plan(int S, int p_lo, int p_hi, int L, int K, long long *n, long long *rec, long long *prof, long long *scratch)
{
    if (S < 1 || S > (1 << 20) || p_lo < 16 || p_lo > p_hi || p_hi > 4096 || L < 1 || L > 12 || K < 1 || K > 11 || (1 << (K - 1)) > p_lo) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    const long long m = 1ll << L, P = p_hi - p_lo + 1;
    if (n) *n = m * p_hi;
    if (rec) *rec = P * m;
    if (prof) *prof = P * m * p_hi;
    if (scratch) *scratch = 8 * S * m * p_hi;
    return MI355_OK;
}

extern "C" {
int mi355_ffa_plan(int S, int p_lo, int p_hi, int L, int K, long long *n, long long *rec, long long *prof, long long *scratch)
{
    return stub_plan(S, p_lo, p_hi, L, K, n, rec, prof, scratch);
}
int mi355_ffa_create(mi355_ctx *ctx, int S, int p_lo, int p_hi, int L, int K, const float *mean, const float *isg, mi355_ffa **out)
{
    if (!ctx || !out || stub_plan(S, p_lo, p_hi, L, K, nullptr, nullptr, nullptr, nullptr)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    *out = new mi355_ffa{S, p_lo, p_hi, L, K, 0, 0, -1, false, mean ? std::vector<float>(mean, mean + S) : std::vector<float>((size_t)S, 0.0f),
                         isg ? std::vector<float>(isg, isg + S) : std::vector<float>((size_t)S, 1.0f)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_ffa_destroy(mi355_ffa *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_ffa_set_stats(mi355_ffa *h, const float *mean, const float *isg)
{
    if (!mean || !isg) { g_err = "invalid argument: stub stats"; return MI355_ERR_INVALID_ARG; }
    h->mean.assign(mean, mean + h->mean.size());
    h->isg.assign(isg, isg + h->isg.size());
    return MI355_OK;
}
int mi355_ffa_get_stats(const mi355_ffa *h, float *mean, float *isg, long long cap)
{
    if (cap < (long long)h->mean.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(mean, h->mean.data(), h->mean.size() * 4);
    memcpy(isg, h->isg.data(), h->isg.size() * 4);
    return MI355_OK;
}
int mi355_ffa_set_generic(mi355_ffa *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_ffa_route(const mi355_ffa *h) { return h->generic ? "generic stub" : "fused stub"; }
int mi355_ffa_work(mi355_ffa *h, const void *in, long long in_pitch, void *peaks, void *profiles)
{
    const long long m = 1ll << h->L, P = h->p_hi - h->p_lo + 1, N = m * h->p_hi;
    if (!in || !peaks || in_pitch < N) { g_err = "invalid argument: stub work"; return MI355_ERR_INVALID_ARG; }
    const float *x = (const float *)in;
    float sum = 0.f;
    for (long long s = 0; s < h->S; s++)
        for (long long t = 0; t < N; t++) sum += x[s * in_pitch + t];  // every float the contract reads
    auto *y = (gr::clenabled::clPeriodSearch::peak *)peaks;
    for (long long i = 0; i < h->S * P * m; i++) y[i] = {(float)(h->calls + 1) + 0.f * sum, (uint32_t)i};
    if (profiles)
        for (long long i = 0; i < h->S * P * m; i++)
            for (long long j = 0; j < h->p_lo + (i / m) % P; j++) ((float *)profiles)[i * h->p_hi + j] = (float)(h->calls + 1);
    h->calls++;
    h->last_pitch = in_pitch;
    h->last_profiles = profiles != nullptr;
    return MI355_OK;
}
double mi355_ffa_period(int p, int L, int i, double tsamp)
{
    if (L < 1 || L > 12 || p < 16 || p > 4096 || i < 0 || i >= (1 << L) || !(tsamp > 0.0)) return NAN;
    return ((double)p + (double)i / (double)((1 << L) - 1)) * tsamp;
}
}

using gr::clenabled::clPeriodSearch;

// one work() call on exact-size heap buffers, as the scheduler makes it: n items in, n items out; returns what work() returned, or -1
// when a record is not the stub's, -2 when a profile float is neither the stub's nor, at j >= p, the prefill
static int call(clPeriodSearch &fs, int n, int first_call, bool profiles, int p_lo, int p_hi, int L)
{
    const size_t in_bytes = (size_t)n * (size_t)fs.input_signature()->sizeof_stream_item(0);
    const size_t out_bytes = (size_t)n * (size_t)fs.output_signature()->sizeof_stream_item(0);
    const size_t prof_bytes = (size_t)n * (size_t)fs.output_signature()->sizeof_stream_item(1);
    std::vector<float> x(in_bytes / 4, 1.0f);
    std::vector<clPeriodSearch::peak> y(out_bytes / sizeof(clPeriodSearch::peak), clPeriodSearch::peak{-7.0f, 0xABCDu});
    std::vector<float> prof(profiles ? prof_bytes / 4 : 0, -3.0f);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    if (profiles) out.push_back(prof.data());
    const int got = fs.work(n, in, out);
    const size_t per = n ? y.size() / (size_t)n : 0, m = (size_t)1 << L, P = (size_t)(p_hi - p_lo + 1);
    for (size_t i = 0; i < y.size(); i++)
        if (y[i].snr != (float)(first_call + (int)(i / per)) || y[i].loc != (uint32_t)(i % per)) return -1;
    for (size_t i = 0; i < prof.size(); i++) {
        const size_t rec = i / (size_t)p_hi, j = i % (size_t)p_hi, p = (size_t)p_lo + (rec % per / m) % P;
        if (prof[i] != (j < p ? (float)(first_call + (int)(rec / per)) : -3.0f)) return -2;
    }
    return got;
}

static int run(int S, int p_lo, int p_hi, int L, int K)
{
    const long long m = 1ll << L, P = p_hi - p_lo + 1, N = m * p_hi;
    std::vector<float> mu((size_t)S), g((size_t)S);
    for (int i = 0; i < S; i++) { mu[(size_t)i] = (float)i; g[(size_t)i] = 1.0f / (float)(i + 1); }
    auto fs = clPeriodSearch::make(1, 2, 0, 0, S, p_lo, p_hi, L, K, mu, g);
    // io signature, item sizes, history
    CHECK(fs->input_signature()->min_streams() == 1 && fs->input_signature()->max_streams() == 1);
    CHECK(fs->output_signature()->min_streams() == 1 && fs->output_signature()->max_streams() == 2);
    CHECK(fs->input_signature()->sizeof_stream_item(0) == 4 * S * N && fs->output_signature()->sizeof_stream_item(0) == 8 * S * P * m);
    CHECK(fs->output_signature()->sizeof_stream_item(1) == 4 * S * P * m * p_hi);
    CHECK(sizeof(clPeriodSearch::peak) == 8);
    CHECK((int)fs->history() == 1 && fs->segment_len() == N && fs->records_per_series() == P * m);
    CHECK(fs->route() == "fused stub" && fs->mean() == mu && fs->inv_sigma() == g);
    CHECK(fs->period(p_lo, (int)m - 1, 2.0) == 2.0 * (p_lo + 1) && std::isnan(fs->period(p_lo, (int)m, 1.0)));
    // what work() hands the library: one call per item, in_pitch N, each item at its own offset of every stream
    int calls = 0;
    for (int n : {1, 2, 3}) {
        CHECK(call(*fs, n, calls + 1, n != 2, p_lo, p_hi, L) == n);
        calls += n;
    }
    CHECK(call(*fs, 0, calls + 1, true, p_lo, p_hi, L) == 0);
    fs->set_generic(true);
    CHECK(fs->route() == "generic stub");
    // set_stats: the sizes are checked by the block; a refused update keeps the old values
    std::vector<float> m2((size_t)S, 2.0f), g2((size_t)S, 0.25f);
    fs->set_stats(m2, g2);
    CHECK(fs->mean() == m2 && fs->inv_sigma() == g2);
    for (size_t bad : {(size_t)0, (size_t)S - 1, (size_t)S + 1, 2 * (size_t)S}) {
        CHECK(throws<std::invalid_argument>([&] { fs->set_stats(std::vector<float>(bad, 0.f), g2); }) && fs->mean() == m2 && fs->inv_sigma() == g2);
        CHECK(throws<std::invalid_argument>([&] { fs->set_stats(m2, std::vector<float>(bad, 0.f)); }) && fs->mean() == m2 && fs->inv_sigma() == g2);
    }
    CHECK(call(*fs, 2, calls + 1, true, p_lo, p_hi, L) == 2);
    // no statistics at make(): mean 0, inv_sigma 1
    auto z = clPeriodSearch::make(1, 2, 0, 0, S, p_lo, p_hi, L, K);
    CHECK(z->mean() == std::vector<float>((size_t)S, 0.0f) && z->inv_sigma() == std::vector<float>((size_t)S, 1.0f));
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 16, 16, 1, 1}, {3, 16, 19, 3, 4}, {2, 37, 40, 5, 5}, {1, 4093, 4096, 4, 6}, {5, 250, 251, 6, 7}}) {
        const int rc = run(s[0], s[1], s[2], s[3], s[4]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{0, 16, 16, 1, 1}, {(1 << 20) + 1, 16, 16, 1, 1}, {1, 15, 16, 1, 1}, {1, 17, 16, 1, 1}, {1, 16, 4097, 1, 1},
                                               {1, 16, 16, 0, 1}, {1, 16, 16, 13, 1}, {1, 16, 16, 1, 0}, {1, 2048, 4096, 1, 12}, {1, 16, 32, 3, 6}};
    for (const auto &s : bad) CHECK(throws<std::invalid_argument>([&] { clPeriodSearch::make(1, 2, 0, 99, s[0], s[1], s[2], s[3], s[4]); }));
    // a stream item of 2 GiB or more: 64 series of 4096 x 4096 floats
    CHECK(throws<std::invalid_argument>([] { clPeriodSearch::make(1, 2, 0, 99, 64, 4096, 4096, 12, 1); }, "2 GiB"));
    // statistics of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([] { clPeriodSearch::make(1, 2, 0, 99, 3, 16, 19, 3, 4, std::vector<float>(7, 0.f)); }));
    CHECK(throws<std::runtime_error>([] { clPeriodSearch::make(1, 2, 0, 99, 3, 16, 19, 3, 4); }, "no such device") && g_live_ctx == 0);
    printf("ffa host ok\n");
    return 0;
}
