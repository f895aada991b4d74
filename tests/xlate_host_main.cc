// Stand-alone program around host/lib/clFreqXlatingFIRFilter_impl.cc for tests/test_xlate_host.py: the block class over a STUB of the C
// ABI, no device.  The stub's mi355_xlate_work reads every input item the contract names (n D + K - 1) and writes n items to each of
// the C output pointers -- the test hands it heap buffers of exactly that size, so under -fsanitize=address,undefined a work() that
// passes one item too few, one output pointer too few or a stale history is caught -- and returns y_c[m] = (calls, c + m / 1024) so that
// the caller can tell which call and channel wrote what.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <cmath>
#include <vector>

struct mi355_xlate {
    int D, K, C, complex_taps, generic;
    long long calls, skipped;
    std::vector<float> taps;
    std::vector<double> freq;
};

extern "C" {
int mi355_xlate_plan(int D, int K, long long n, long long *nin, int *history)
{
    if (D < 1 || K < 1 || n < 0) { g_err = "invalid argument: stub plan"; return MI355_ERR_INVALID_ARG; }
    if (nin) *nin = n == 0 ? 0 : n * D + K - 1;
    if (history) *history = K;
    return MI355_OK;
}
int mi355_xlate_create(mi355_ctx *ctx, int D, const void *taps, int K, int complex_taps, double fs, const double *freqs, int nfreq, int,
                       mi355_xlate **out)
{
    if (!ctx || !out || !taps || !freqs || nfreq < 1 || !(fs > 0)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    for (int c = 0; c < nfreq; c++)
        if (!std::isfinite(freqs[c])) { g_err = "invalid argument: stub frequency"; return MI355_ERR_INVALID_ARG; }
    const float *t = (const float *)taps;
    *out = new mi355_xlate{D, K, nfreq, complex_taps, 0, 0, 0, std::vector<float>(t, t + (size_t)K * (complex_taps ? 2 : 1)),
                           std::vector<double>(freqs, freqs + nfreq)};
    return MI355_OK;
}
int mi355_xlate_destroy(mi355_xlate *h) { delete h; return MI355_OK; }
int mi355_xlate_set_taps(mi355_xlate *h, const void *taps, int K)
{
    if (K < 1) { g_err = "invalid argument: stub taps"; return MI355_ERR_INVALID_ARG; }
    const float *t = (const float *)taps;
    h->taps.assign(t, t + (size_t)K * (h->complex_taps ? 2 : 1));
    h->K = K;
    return MI355_OK;
}
int mi355_xlate_ntaps(const mi355_xlate *h) { return h->K; }
int mi355_xlate_get_taps(const mi355_xlate *h, void *out, int cap)
{
    if (cap < h->K) return MI355_ERR_INVALID_ARG;
    memcpy(out, h->taps.data(), h->taps.size() * sizeof(float));
    return h->K;
}
int mi355_xlate_set_center_freq(mi355_xlate *h, int c, double f)
{
    if (c < 0 || c >= h->C || !std::isfinite(f)) { g_err = "invalid argument: stub retune"; return MI355_ERR_INVALID_ARG; }
    h->freq[c] = f;
    return MI355_OK;
}
int mi355_xlate_get_center_freq(const mi355_xlate *h, int c, double *f)
{
    if (c < 0 || c >= h->C) { g_err = "invalid argument: stub channel"; return MI355_ERR_INVALID_ARG; }
    *f = h->freq[c];
    return MI355_OK;
}
int mi355_xlate_skip(mi355_xlate *h, long long n)
{
    if (n < 0) { g_err = "invalid argument: stub skip"; return MI355_ERR_INVALID_ARG; }
    h->skipped += n;
    return MI355_OK;
}
int mi355_xlate_set_generic(mi355_xlate *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_xlate_route(const mi355_xlate *h) { return h->generic ? "generic stub" : "fused stub"; }
int mi355_xlate_work(mi355_xlate *h, long long n, const void *in, void *const *outs)
{
    const float *x = (const float *)in;
    float sum = 0.f;
    for (long long i = 0; n > 0 && i < 2 * (n * h->D + h->K - 1); i++) sum += x[i];  // every item the contract reads
    for (int c = 0; c < h->C; c++) {
        float *y = (float *)outs[c];
        for (long long m = 0; m < n; m++) {
            y[2 * m] = (float)h->calls + 0.f * sum;
            y[2 * m + 1] = (float)c + (float)m / 1024.f;
        }
    }
    h->calls++;
    return MI355_OK;
}
}

using gr::clenabled::clFreqXlatingFIRFilter;

// one work() call on exact-size heap buffers; returns what work() returned, or -1 when a written value is not the stub's
static int call(clFreqXlatingFIRFilter &fx, int n, int call_no)
{
    const int C = fx.num_channels(), D = (int)fx.decimation(), hist = (int)fx.history();
    std::vector<gr_complex> x((size_t)n * D + hist - 1, gr_complex(1.f, -1.f));
    std::vector<std::vector<gr_complex>> y((size_t)C, std::vector<gr_complex>((size_t)n, gr_complex(-7.f, -7.f)));
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out;
    for (auto &v : y) out.push_back(v.data());
    const int got = fx.work(n, in, out);
    for (int c = 0; c < C && got > 0; c++)
        for (int m = 0; m < n; m++)
            if (y[c][m] != gr_complex((float)call_no, (float)c + (float)m / 1024.f)) return -1;
    for (int c = 0; c < C && got == 0; c++)
        for (int m = 0; m < n; m++)
            if (y[c][m] != gr_complex(-7.f, -7.f)) return -1;
    return got;
}

static int run(int D, int K, int C, bool cplx)
{
    std::vector<double> f;
    for (int c = 0; c < C; c++) f.push_back(1000.0 * c - 500.0);
    auto fx = cplx ? clFreqXlatingFIRFilter::make_ccc(1, 2, 0, 0, D, std::vector<gr_complex>((size_t)K, gr_complex(0.5f, -0.25f)), f, 48000.0)
                   : clFreqXlatingFIRFilter::make(1, 2, 0, 0, D, std::vector<float>((size_t)K, 0.5f), f, 48000.0, true);
    CHECK(fx->num_channels() == C && (int)fx->decimation() == D && (int)fx->history() == K && fx->route() == "fused stub");
    CHECK(fx->input_signature()->max_streams() == 1 && fx->output_signature()->min_streams() == C && fx->output_signature()->max_streams() == C);
    CHECK(fx->message_ports_in().size() == 1 && fx->message_ports_in()[0] == "freq");
    CHECK((int)fx->taps().size() == K && fx->taps()[0] == (cplx ? gr_complex(0.5f, -0.25f) : gr_complex(0.5f, 0.f)));
    for (int c = 0; c < C; c++) CHECK(fx->center_freq(c) == f[c]);
    int calls = 0;
    for (int n : {1, 2, 64, 257}) CHECK(call(*fx, n, calls++) == n);
    // the "freq" port retunes channel 0 only
    CHECK(fx->post_double("freq", 12345.5) && fx->center_freq(0) == 12345.5);
    for (int c = 1; c < C; c++) CHECK(fx->center_freq(c) == f[c]);
    CHECK(!fx->post_double("other", 1.0));
    fx->set_center_freq(-77.0, C - 1);
    CHECK(fx->center_freq(C - 1) == -77.0);
    CHECK(throws<std::invalid_argument>([&] { fx->set_center_freq(1.0, C); }));
    CHECK(throws<std::invalid_argument>([&] { fx->set_center_freq(std::nan(""), 0); }));
    fx->set_generic(true);
    CHECK(fx->route() == "generic stub");
    fx->skip(1ll << 40);
    CHECK(call(*fx, 5, calls++) == 5);
    // new taps: the work() call after set_taps() installs the new history and produces nothing; the next one runs with it
    int prev = K;
    for (int K2 : {K + 9, 1, K}) {
        fx->set_taps(std::vector<gr_complex>((size_t)K2, gr_complex(0.25f, 0.f)));
        CHECK((int)fx->history() == prev);  // (still the old one)
        prev = K2;
        CHECK(call(*fx, 3, calls) == 0 && (int)fx->history() == K2);
        CHECK(call(*fx, 33, calls++) == 33);
    }
    if (!cplx) CHECK(throws<std::invalid_argument>([&] { fx->set_taps(std::vector<gr_complex>(3, gr_complex(1.f, 1.f))); }) && (int)fx->history() == K);
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 1, 1, 0}, {16, 65, 8, 0}, {3, 7, 2, 1}, {64, 131, 3, 1}}) {
        const int rc = run(s[0], s[1], s[2], s[3] != 0);
        if (rc) return rc;
    }
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<float> t(5, 1.f);
    CHECK(throws<std::invalid_argument>([&] { clFreqXlatingFIRFilter::make(1, 2, 0, 99, 0, t, {0.0}, 1e6); }));
    CHECK(throws<std::invalid_argument>([&] { clFreqXlatingFIRFilter::make(1, 2, 0, 99, 4, std::vector<float>(), {0.0}, 1e6); }));
    CHECK(throws<std::invalid_argument>([&] { clFreqXlatingFIRFilter::make(1, 2, 0, 99, 4, t, {}, 1e6); }));
    CHECK(throws<std::invalid_argument>([&] { clFreqXlatingFIRFilter::make(1, 2, 0, 0, 4, t, {0.0}, 0.0); }));
    CHECK(throws<std::invalid_argument>([&] { clFreqXlatingFIRFilter::make(1, 2, 0, 0, 4, t, {0.0, std::nan("")}, 1e6); }));
    CHECK(throws<std::runtime_error>([&] { clFreqXlatingFIRFilter::make(1, 2, 0, 99, 4, t, {0.0}, 1e6); }, "no such device"));
    printf("xlate host ok\n");
    return 0;
}
