// Stand-alone program around host/lib/clSpectralSearch_impl.cc for tests/test_ssearch_host.py: the block class over a STUB of the C
// ABI, no device.  The stub's mi355_ssearch_work reads every input float the contract names (S series of n floats at in_pitch) and
// writes every peak record (S n / 2 / block_bins) and, if asked, every spectrum float (S n / 2) -- the test hands it heap buffers of
// exactly the item sizes, so under -fsanitize=address,undefined a work() that passes a wrong pointer, a wrong pitch or a wrong item
// offset is caught -- and records what it was handed.  The stub's plan and freq are the contract's arithmetic, written out again here.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <cmath>
#include <vector>

struct mi355_ssearch {
    int S, n, H, Bb, k_lo, kind, generic;
    long long calls, last_pitch;
    bool last_spectrum;
    std::vector<float> isg;
};

static bool pow2(long long v) { return v > 0 && (v & (v - 1)) == 0; }

static int stub_plan(int S, int n, int H, int Bb, int k_lo, int kind, long long *bins, long long *rec, long long *scratch)
{
    if (S < 1 || S > (1 << 20) || !pow2(n) || n < 256 || n > (1 << 22) || H < 0 || H > 5 || !pow2(Bb) || Bb < 16 || Bb > n / 2 || k_lo < 1 ||
        k_lo > n / 2 - 1 || kind < 0 || kind > 1) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (bins) *bins = n / 2;
    if (rec) *rec = n / 2 / Bb;
    if (scratch) *scratch = kind == MI355_SSEARCH_SERIES ? 10ll * n : 0;
    return MI355_OK;
}

extern "C" {
int mi355_ssearch_plan(int S, int n, int H, int Bb, int k_lo, int kind, long long *bins, long long *rec, long long *scratch)
{
    return stub_plan(S, n, H, Bb, k_lo, kind, bins, rec, scratch);
}
int mi355_ssearch_create(mi355_ctx *ctx, int S, int n, int H, int Bb, int k_lo, int kind, const float *isg, mi355_ssearch **out)
{
    if (!ctx || !out || stub_plan(S, n, H, Bb, k_lo, kind, nullptr, nullptr, nullptr)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    *out = new mi355_ssearch{S, n, H, Bb, k_lo, kind, 0, 0, -1, false, isg ? std::vector<float>(isg, isg + S) : std::vector<float>((size_t)S, 1.0f)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_ssearch_destroy(mi355_ssearch *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_ssearch_set_stats(mi355_ssearch *h, const float *isg)
{
    if (!isg) { g_err = "invalid argument: stub stats"; return MI355_ERR_INVALID_ARG; }
    h->isg.assign(isg, isg + h->isg.size());
    return MI355_OK;
}
int mi355_ssearch_get_stats(const mi355_ssearch *h, float *isg, long long cap)
{
    if (cap < (long long)h->isg.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(isg, h->isg.data(), h->isg.size() * 4);
    return MI355_OK;
}
int mi355_ssearch_set_generic(mi355_ssearch *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_ssearch_route(const mi355_ssearch *h) { return h->generic ? "generic stub" : "tiled stub"; }
int mi355_ssearch_work(mi355_ssearch *h, const void *in, long long in_pitch, void *peaks, void *spectrum, void *cands, long long max_cands, void *counts)
{
    const long long N = h->n, Nb = N / 2, rec = Nb / h->Bb;
    if (!in || !peaks || in_pitch < N || cands || counts || max_cands) { g_err = "invalid argument: stub work"; return MI355_ERR_INVALID_ARG; }
    const float *x = (const float *)in;
    float sum = 0.f;
    for (long long s = 0; s < h->S; s++)
        for (long long t = 0; t < N; t++) sum += x[s * in_pitch + t];  // every float the contract reads
    auto *y = (gr::clenabled::clSpectralSearch::peak *)peaks;
    for (long long i = 0; i < h->S * rec; i++) y[i] = {(float)(h->calls + 1) + 0.f * sum, (uint32_t)i};
    if (spectrum)
        for (long long i = 0; i < h->S * Nb; i++) ((float *)spectrum)[i] = (float)(h->calls + 1);
    h->calls++;
    h->last_pitch = in_pitch;
    h->last_spectrum = spectrum != nullptr;
    return MI355_OK;
}
double mi355_ssearch_freq(int n, double tsamp, int h, int k)
{
    if (!pow2(n) || n < 256 || n > (1 << 22) || h < 0 || h > 5 || k < 0 || k >= n / 2 || !(tsamp > 0.0) || !std::isfinite(tsamp)) return NAN;
    return (double)k / ((double)(1 << h) * (double)n * tsamp);
}
}

using gr::clenabled::clSpectralSearch;

// one work() call on exact-size heap buffers, as the scheduler makes it: n items in, n items out; returns what work() returned, or -1
// when a record is not the stub's, -2 when a spectrum float is not
static int call(clSpectralSearch &ss, int n, int first_call, bool spectrum)
{
    const size_t in_bytes = (size_t)n * (size_t)ss.input_signature()->sizeof_stream_item(0);
    const size_t out_bytes = (size_t)n * (size_t)ss.output_signature()->sizeof_stream_item(0);
    const size_t spec_bytes = (size_t)n * (size_t)ss.output_signature()->sizeof_stream_item(1);
    std::vector<float> x(in_bytes / 4, 1.0f);
    std::vector<clSpectralSearch::peak> y(out_bytes / sizeof(clSpectralSearch::peak), clSpectralSearch::peak{-7.0f, 0xABCDu});
    std::vector<float> w(spectrum ? spec_bytes / 4 : 0, -3.0f);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    if (spectrum) out.push_back(w.data());
    const int got = ss.work(n, in, out);
    const size_t per = n ? y.size() / (size_t)n : 0, wper = n ? w.size() / (size_t)n : 0;
    for (size_t i = 0; i < y.size(); i++)
        if (y[i].snr != (float)(first_call + (int)(i / per)) || y[i].loc != (uint32_t)(i % per)) return -1;
    for (size_t i = 0; i < w.size(); i++)
        if (w[i] != (float)(first_call + (int)(i / wper))) return -2;
    return got;
}

static int run(int S, int n, int H, int Bb, int k_lo)
{
    const long long Nb = n / 2, rec = Nb / Bb;
    std::vector<float> g((size_t)S);
    for (int i = 0; i < S; i++) g[(size_t)i] = 1.0f / (float)(i + 1);
    auto ss = clSpectralSearch::make(1, 2, 0, 0, S, n, H, Bb, k_lo, g);
    // io signature, item sizes, history
    CHECK(ss->input_signature()->min_streams() == 1 && ss->input_signature()->max_streams() == 1);
    CHECK(ss->output_signature()->min_streams() == 1 && ss->output_signature()->max_streams() == 2);
    CHECK(ss->input_signature()->sizeof_stream_item(0) == 4 * S * n && ss->output_signature()->sizeof_stream_item(0) == 8 * S * rec);
    CHECK(ss->output_signature()->sizeof_stream_item(1) == 4 * S * Nb);
    CHECK(sizeof(clSpectralSearch::peak) == 8);
    CHECK((int)ss->history() == 1 && ss->segment_len() == n && ss->num_bins() == Nb && ss->records_per_series() == rec);
    CHECK(ss->route() == "tiled stub" && ss->inv_sigma() == g);
    CHECK(ss->freq(1, 2, 1.0) == 1.0 / n && std::isnan(ss->freq(6, 2, 1.0)) && std::isnan(ss->freq(0, (int)Nb, 1.0)));
    // what work() hands the library: one call per item, in_pitch n, each item at its own offset of every stream
    int calls = 0;
    for (int m : {1, 2, 3}) {
        CHECK(call(*ss, m, calls + 1, m != 2) == m);
        calls += m;
    }
    CHECK(call(*ss, 0, calls + 1, true) == 0);
    ss->set_generic(true);
    CHECK(ss->route() == "generic stub");
    // set_stats: the size is checked by the block; a refused update keeps the old values
    std::vector<float> g2((size_t)S, 0.25f);
    ss->set_stats(g2);
    CHECK(ss->inv_sigma() == g2);
    for (size_t bad : {(size_t)0, (size_t)S - 1, (size_t)S + 1, 2 * (size_t)S})
        CHECK(throws<std::invalid_argument>([&] { ss->set_stats(std::vector<float>(bad, 0.f)); }) && ss->inv_sigma() == g2);
    CHECK(call(*ss, 2, calls + 1, true) == 2);
    // no statistics at make(): inv_sigma 1
    auto z = clSpectralSearch::make(1, 2, 0, 0, S, n, H, Bb, k_lo);
    CHECK(z->inv_sigma() == std::vector<float>((size_t)S, 1.0f));
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 256, 0, 16, 1}, {3, 256, 5, 128, 127}, {2, 16384, 5, 256, 8}, {5, 4096, 3, 2048, 2}, {1, 1 << 20, 5, 1024, 16}}) {
        const int rc = run(s[0], s[1], s[2], s[3], s[4]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{0, 256, 0, 16, 1}, {(1 << 20) + 1, 256, 0, 16, 1}, {1, 128, 0, 16, 1}, {1, 4095, 0, 16, 1},
                                               {1, 1 << 23, 0, 16, 1}, {1, 256, -1, 16, 1}, {1, 256, 6, 16, 1}, {1, 256, 0, 8, 1},
                                               {1, 256, 0, 48, 1}, {1, 256, 0, 256, 1}, {1, 256, 0, 16, 0}, {1, 256, 0, 16, 128}};
    for (const auto &s : bad) CHECK(throws<std::invalid_argument>([&] { clSpectralSearch::make(1, 2, 0, 99, s[0], s[1], s[2], s[3], s[4]); }));
    // a stream item of 2 GiB or more: 512 series of 2^20 floats
    CHECK(throws<std::invalid_argument>([] { clSpectralSearch::make(1, 2, 0, 99, 512, 1 << 20, 5, 1024, 1); }, "2 GiB"));
    // statistics of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([] { clSpectralSearch::make(1, 2, 0, 99, 3, 256, 5, 16, 1, std::vector<float>(7, 0.f)); }));
    CHECK(throws<std::runtime_error>([] { clSpectralSearch::make(1, 2, 0, 99, 3, 256, 5, 16, 1); }, "no such device") && g_live_ctx == 0);
    printf("ssearch host ok\n");
    return 0;
}
