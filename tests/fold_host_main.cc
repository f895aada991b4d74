// Stand-alone program around host/lib/clFolder_impl.cc for tests/test_fold_host.py: the block class over a STUB of the C ABI, no device.
// The stub's mi355_fold_work reads every input float and flag byte the contract names (n R F floats, n R bytes) and writes every output
// it is handed (n / Ts x R nbin F floats, n / Ts x R nbin counts) -- the test hands the block heap buffers of exactly the scheduler's
// sizes, so under -fsanitize=address,undefined a work() that passes a wrong count or a short buffer is caught -- and records what it
// was handed.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <vector>

struct mi355_fold {
    int R, F, nbin, Ts, generic;
    unsigned long long T0;
    long long calls, last_n;
    bool had_tflags, had_hits;
    std::vector<uint64_t> models;
};

static int stub_plan(int R, int F, int nbin, int Ts, long long *a, long long *b, long long *c)
{
    if (R < 1 || R > 4096 || F < 1 || F > 16384 || nbin < 2 || nbin > 4096 || Ts < 16 || Ts > 16384 || Ts % 16) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (a) *a = (long long)R * F;
    if (b) *b = (long long)R * nbin * F;
    if (c) *c = (long long)R * nbin;
    return MI355_OK;
}

extern "C" {
int mi355_fold_plan(int R, int F, int nbin, int Ts, long long *a, long long *b, long long *c) { return stub_plan(R, F, nbin, Ts, a, b, c); }
int mi355_fold_create(mi355_ctx *ctx, int R, int F, int nbin, int Ts, const uint64_t *models, mi355_fold **out)
{
    if (!ctx || !out || !models || stub_plan(R, F, nbin, Ts, nullptr, nullptr, nullptr)) {
        g_err = "invalid argument: stub create";
        return MI355_ERR_INVALID_ARG;
    }
    *out = new mi355_fold{R, F, nbin, Ts, 0, 0, 0, 0, false, false, std::vector<uint64_t>(models, models + 3 * (size_t)R)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_fold_destroy(mi355_fold *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
// the stub refuses a table whose first word is all ones: the way the test makes an update fail
int mi355_fold_set_models(mi355_fold *h, const uint64_t *models)
{
    if (!models || models[0] == UINT64_MAX) { g_err = "invalid argument: stub models"; return MI355_ERR_INVALID_ARG; }
    h->models.assign(models, models + 3 * (size_t)h->R);
    return MI355_OK;
}
int mi355_fold_get_models(const mi355_fold *h, uint64_t *out, long long cap)
{
    if (cap < (long long)h->models.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(out, h->models.data(), h->models.size() * 8);
    return MI355_OK;
}
int mi355_fold_sample(const mi355_fold *h, unsigned long long *T) { *T = h->T0; return MI355_OK; }
int mi355_fold_set_sample(mi355_fold *h, unsigned long long T) { h->T0 = T; return MI355_OK; }
int mi355_fold_skip(mi355_fold *h, long long n)
{
    if (n < 0) { g_err = "invalid argument: stub skip"; return MI355_ERR_INVALID_ARG; }
    h->T0 += (unsigned long long)n;
    return MI355_OK;
}
int mi355_fold_set_generic(mi355_fold *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_fold_route(const mi355_fold *h) { return h->generic ? "generic stub" : "bins stub"; }
int mi355_fold_work(mi355_fold *h, long long n, const void *in, const void *tflags, void *out, void *hits)
{
    if (n <= 0 || n % h->Ts || !in || !out) { g_err = "invalid argument: stub work"; return MI355_ERR_INVALID_ARG; }
    const long long RF = (long long)h->R * h->F, ns = n / h->Ts, RB = (long long)h->R * h->nbin;
    const float *x = (const float *)in;
    float sum = 0.0f;
    for (long long i = 0; i < n * RF; i++) sum += x[i];  // every float the contract reads
    long long flagged = 0;
    if (tflags)
        for (long long i = 0; i < n * h->R; i++) flagged += ((const uint8_t *)tflags)[i] != 0;
    float *y = (float *)out;
    for (long long i = 0; i < ns * RB * h->F; i++) y[i] = sum / (float)(n * RF) + (float)(h->calls + 1) + (float)flagged;  // 1 + call number + flags
    if (hits)
        for (long long i = 0; i < ns * RB; i++) ((uint32_t *)hits)[i] = (uint32_t)(i / RB + 1);  // the sub-integration's number within the call, plus one
    h->calls++;
    h->last_n = n;
    h->T0 += (unsigned long long)n;
    h->had_tflags = tflags != nullptr;
    h->had_hits = hits != nullptr;
    return MI355_OK;
}
}

using gr::clenabled::clFolder;

// one work() call for ns output items on exact-size heap buffers, as the scheduler makes it, with `nin` input and `nout` output streams;
// `flagged` of the flag bytes are set.  Returns what work() returned, or -1 when an output is not the stub's
static int call(clFolder &fo, int ns, int nin, int nout, int call_no, int flagged)
{
    const size_t Ts = fo.decimation();
    const size_t isz = (size_t)fo.input_signature()->sizeof_stream_item(0), fsz = (size_t)fo.input_signature()->sizeof_stream_item(1);
    const size_t osz = (size_t)fo.output_signature()->sizeof_stream_item(0), hsz = (size_t)fo.output_signature()->sizeof_stream_item(1);
    std::vector<float> x((size_t)ns * Ts * isz / 4, 1.0f), y((size_t)ns * osz / 4, -7.0f);
    std::vector<uint8_t> tf((size_t)ns * Ts * fsz, 0);
    for (int i = 0; i < flagged; i++) tf[tf.size() - 1 - (size_t)i] = 1;  // the last bytes: a short read would miss them
    std::vector<uint32_t> hits((size_t)ns * hsz / 4, 0xEEEEEEEEu);
    gr_vector_const_void_star in = {x.data()};
    if (nin >= 2) in.push_back(tf.data());
    gr_vector_void_star out = {y.data()};
    if (nout >= 2) out.push_back(hits.data());
    const int got = fo.work(ns, in, out);
    const float want = 1.0f + (float)call_no + (nin >= 2 ? (float)flagged : 0.0f);
    for (size_t i = 0; i < y.size(); i++)
        if (y[i] != want) return -1;
    for (size_t i = 0; i < hits.size(); i++)
        if (hits[i] != (nout >= 2 ? (uint32_t)(i / (hsz / 4) + 1) : 0xEEEEEEEEu)) return -1;
    return got;
}

static int run(int R, int F, int nbin, int Ts)
{
    std::vector<uint64_t> models(3 * (size_t)R);
    for (size_t i = 0; i < models.size(); i++) models[i] = 1000 + i;
    auto fo = clFolder::make(1, 2, 0, 0, R, F, nbin, Ts, models);
    // io signature, item sizes, decimation, history, the message port
    CHECK(fo->input_signature()->min_streams() == 1 && fo->input_signature()->max_streams() == 2);
    CHECK(fo->output_signature()->min_streams() == 1 && fo->output_signature()->max_streams() == 2);
    CHECK(fo->input_signature()->sizeof_stream_item(0) == 4 * R * F && fo->input_signature()->sizeof_stream_item(1) == R);
    CHECK(fo->output_signature()->sizeof_stream_item(0) == 4 * R * nbin * F && fo->output_signature()->sizeof_stream_item(1) == 4 * R * nbin);
    CHECK((int)fo->history() == 1 && (int)fo->decimation() == Ts && fo->subint_len() == Ts && fo->nbin() == nbin && fo->output_multiple() == 1);
    CHECK(fo->route() == "bins stub" && fo->models() == models && fo->sample() == 0);
    CHECK(fo->message_ports_in() == std::vector<std::string>{"models"});
    // what work() hands the library: ns Ts samples, the optional streams only when they are connected
    int calls = 0;
    unsigned long long T = 0;
    for (int nin : {1, 2})
        for (int nout : {1, 2})
            for (int ns : {1, 3}) {
                CHECK(call(*fo, ns, nin, nout, ++calls, 2) == ns);
                T += (unsigned long long)ns * Ts;
                CHECK(fo->sample() == T);
            }
    CHECK(call(*fo, 0, 2, 2, calls, 0) == 0 && fo->sample() == T);  // nothing asked: nothing is done
    fo->set_sample(UINT64_MAX - 5);
    fo->skip(10);
    CHECK(fo->sample() == 4);  // the counter wraps
    CHECK(throws<std::invalid_argument>([&] { fo->skip(-1); }) && fo->sample() == 4);
    fo->set_generic(true);
    CHECK(fo->route() == "generic stub");
    // set_models: the size is checked by the block, and a refused update keeps the old table
    std::vector<uint64_t> m2(models.size(), 7);
    fo->set_models(m2);
    CHECK(fo->models() == m2);
    for (size_t bad : {(size_t)0, models.size() - 1, models.size() + 1}) {
        CHECK(throws<std::invalid_argument>([&] { fo->set_models(std::vector<uint64_t>(bad, 0)); }) && fo->models() == m2);
    }
    CHECK(throws<std::invalid_argument>([&] { fo->set_models(std::vector<uint64_t>(models.size(), UINT64_MAX)); }) && fo->models() == m2);  // the library refused it
    // the message port: a table of the right size is installed, any other message is dropped without a throw
    CHECK(fo->post_u64vector("models", models) && fo->models() == models);
    CHECK(fo->post_u64vector("models", std::vector<uint64_t>(models.size() + 3, 1)) && fo->models() == models);
    CHECK(!fo->post_u64vector("freq", models));
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 1, 2, 16}, {2, 5, 3, 32}, {3, 52, 7, 48}, {2, 256, 16, 64}}) {
        const int rc = run(s[0], s[1], s[2], s[3]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<uint64_t> m(6, 0);
    const std::vector<std::vector<int>> bad = {{0, 8, 4, 16}, {4097, 8, 4, 16}, {2, 0, 4, 16}, {2, 16385, 4, 16}, {2, 8, 1, 16}, {2, 8, 4097, 16},
                                               {2, 8, 4, 0}, {2, 8, 4, 24}, {2, 8, 4, 16400}};
    for (const auto &s : bad) CHECK(throws<std::invalid_argument>([&] { clFolder::make(1, 2, 0, 99, s[0], s[1], s[2], s[3], m); }));
    // models of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([&] { clFolder::make(1, 2, 0, 99, 2, 8, 4, 16, std::vector<uint64_t>(5, 0)); }));
    CHECK(throws<std::runtime_error>([&] { clFolder::make(1, 2, 0, 99, 2, 8, 4, 16, m); }, "no such device") && g_live_ctx == 0);
    // an output item of 2 GiB or more is no stream item
    CHECK(throws<std::invalid_argument>([&] { clFolder::make(1, 2, 0, 0, 4096, 16384, 4096, 16, std::vector<uint64_t>(3 * 4096, 0)); }));
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    printf("fold host ok\n");
    return 0;
}
