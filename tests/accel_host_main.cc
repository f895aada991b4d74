// Stand-alone program around host/lib/clAccelResampler_impl.cc for tests/test_accel_host.py: the block class over a STUB of the C ABI,
// no device.  The stub's mi355_accel_work reads every input word the contract names (S series of n words at in_pitch) and writes every
// output word (S na rows of n words at out_pitch) -- the test hands it heap buffers of exactly the item sizes, so under
// -fsanitize=address,undefined a work() that passes a wrong pointer, a wrong pitch, a wrong trial range or a wrong item offset is
// caught -- and records what it was handed.  The stub's plan and coefficient bound are the contract's arithmetic, written out again here.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <vector>

struct mi355_accel {
    int S, n, A, generic;
    long long calls, last_in_pitch, last_out_pitch;
    int last_a0, last_na;
    std::vector<long long> c;
};

static bool coeff_ok(long long c, long long n)
{
    const unsigned __int128 m = c < 0 ? (unsigned __int128)(-(__int128)c) : (unsigned __int128)c;
    return m * (unsigned __int128)n <= ((unsigned __int128)1 << 63);
}

static int stub_plan(int S, int n, int A, long long *rows, long long *tile, long long *table)
{
    if (S < 1 || S > (1 << 20) || n < 256 || n > (1 << 22) || A < 1 || A > 4096) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (rows) *rows = (long long)S * A;
    if (tile) *tile = 1024;
    if (table) *table = 8ll * A;
    return MI355_OK;
}

extern "C" {
int mi355_accel_plan(int S, int n, int A, long long *rows, long long *tile, long long *table) { return stub_plan(S, n, A, rows, tile, table); }
int mi355_accel_create(mi355_ctx *ctx, int S, int n, int A, const long long *c, mi355_accel **out)
{
    if (!ctx || !out || stub_plan(S, n, A, nullptr, nullptr, nullptr)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    for (int a = 0; c && a < A; a++)
        if (!coeff_ok(c[a], n)) { g_err = "invalid argument: stub coefficient"; return MI355_ERR_INVALID_ARG; }
    *out = new mi355_accel{S, n, A, 0, 0, -1, -1, -1, -1, c ? std::vector<long long>(c, c + A) : std::vector<long long>((size_t)A, 0ll)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_accel_destroy(mi355_accel *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_accel_set_trials(mi355_accel *h, const long long *c)
{
    if (!c) { g_err = "invalid argument: stub trials"; return MI355_ERR_INVALID_ARG; }
    for (int a = 0; a < h->A; a++)
        if (!coeff_ok(c[a], h->n)) { g_err = "invalid argument: stub coefficient"; return MI355_ERR_INVALID_ARG; }
    h->c.assign(c, c + h->A);
    return MI355_OK;
}
int mi355_accel_get_trials(const mi355_accel *h, long long *c, long long cap)
{
    if (cap < (long long)h->c.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(c, h->c.data(), h->c.size() * 8);
    return MI355_OK;
}
int mi355_accel_set_generic(mi355_accel *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_accel_route(const mi355_accel *h) { return h->generic ? "generic stub" : "tiled stub"; }
int mi355_accel_work(mi355_accel *h, const void *in, long long in_pitch, void *out, long long out_pitch, int a0, int na)
{
    const long long N = h->n;
    if (!in || !out || in_pitch < N || out_pitch < N || a0 < 0 || na < 1 || a0 + na > h->A) { g_err = "invalid argument: stub work"; return MI355_ERR_INVALID_ARG; }
    const uint32_t *x = (const uint32_t *)in;
    uint32_t sum = 0;
    for (long long s = 0; s < h->S; s++)
        for (long long t = 0; t < N; t++) sum += x[s * in_pitch + t];  // every word the contract reads
    uint32_t *y = (uint32_t *)out;
    for (long long r = 0; r < (long long)h->S * na; r++)
        for (long long t = 0; t < N; t++) y[r * out_pitch + t] = (uint32_t)((h->calls + 1) * 1000 + r) + 0u * sum;
    h->calls++;
    h->last_in_pitch = in_pitch; h->last_out_pitch = out_pitch; h->last_a0 = a0; h->last_na = na;
    return MI355_OK;
}
}

using gr::clenabled::clAccelResampler;

// one work() call on exact-size heap buffers, as the scheduler makes it: n items in, n items out; returns what work() returned, or -1
// when an output word is not the stub's
static int call(clAccelResampler &ar, int n, int first_call)
{
    const size_t in_bytes = (size_t)n * (size_t)ar.input_signature()->sizeof_stream_item(0);
    const size_t out_bytes = (size_t)n * (size_t)ar.output_signature()->sizeof_stream_item(0);
    std::vector<uint32_t> x(in_bytes / 4, 1u), y(out_bytes / 4, 0xABCDu);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    const int got = ar.work(n, in, out);
    const size_t per = n ? y.size() / (size_t)n : 0, N = (size_t)ar.segment_len();
    for (size_t i = 0; i < y.size(); i++)
        if (y[i] != (uint32_t)((size_t)(first_call + (int)(i / per)) * 1000 + (i % per) / N)) return -1;
    return got;
}

static int run(int S, int n, int A)
{
    std::vector<long long> c((size_t)A);
    const long long top = (long long)((1ull << 63) / (unsigned)n);
    for (int a = 0; a < A; a++) c[(size_t)a] = a == 0 ? top : a == 1 ? -top : (long long)a - 3;
    auto ar = clAccelResampler::make(1, 2, 0, 0, S, n, c);
    // io signature, item sizes, history
    CHECK(ar->input_signature()->min_streams() == 1 && ar->input_signature()->max_streams() == 1);
    CHECK(ar->output_signature()->min_streams() == 1 && ar->output_signature()->max_streams() == 1);
    CHECK(ar->input_signature()->sizeof_stream_item(0) == 4 * S * n && ar->output_signature()->sizeof_stream_item(0) == 4 * S * A * n);
    CHECK((int)ar->history() == 1 && ar->segment_len() == n && ar->num_trials() == A && ar->rows() == (long long)S * A);
    CHECK(ar->route() == "tiled stub" && ar->trials() == c);
    // what work() hands the library: one call per item, both pitches n, the whole trial range, each item at its own offset
    int calls = 0;
    for (int m : {1, 2, 3}) {
        CHECK(call(*ar, m, calls + 1) == m);
        calls += m;
    }
    CHECK(call(*ar, 0, calls + 1) == 0);
    ar->set_generic(true);
    CHECK(ar->route() == "generic stub");
    // set_trials: the size is checked by the block, the bound by the library; a refused update keeps the old table
    std::vector<long long> c2((size_t)A, 7);
    ar->set_trials(c2);
    CHECK(ar->trials() == c2);
    for (size_t bad : {(size_t)0, (size_t)A - 1, (size_t)A + 1, 2 * (size_t)A})
        CHECK(throws<std::invalid_argument>([&] { ar->set_trials(std::vector<long long>(bad, 0)); }) && ar->trials() == c2);
    CHECK(throws<std::invalid_argument>([&] { ar->set_trials(std::vector<long long>((size_t)A, top + 1)); }) && ar->trials() == c2);
    CHECK(call(*ar, 2, calls + 1) == 2);
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{1, 256, 1}, {3, 4099, 8}, {2, 8192, 5}, {5, 300, 2}, {1, 1 << 20, 3}}) {
        const int rc = run(s[0], s[1], s[2]);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{0, 256, 1}, {(1 << 20) + 1, 256, 1}, {1, 255, 1}, {1, (1 << 22) + 1, 1}, {1, 256, 0}, {1, 256, 4097},
                                               {1, 256, 70000}};
    for (const auto &s : bad)
        CHECK(throws<std::invalid_argument>([&] { clAccelResampler::make(1, 2, 0, 99, s[0], s[1], std::vector<long long>((size_t)s[2], 0)); }));
    // a stream item of 2 GiB or more: 64 series of 2^20 words, 8 trials
    CHECK(throws<std::invalid_argument>([] { clAccelResampler::make(1, 2, 0, 99, 64, 1 << 20, std::vector<long long>(8, 0)); }, "2 GiB"));
    CHECK(throws<std::runtime_error>([] { clAccelResampler::make(1, 2, 0, 99, 3, 256, std::vector<long long>(2, 0)); }, "no such device") && g_live_ctx == 0);
    // a coefficient outside the bound is the library's refusal: an argument error, and nothing stays alive
    CHECK(throws<std::invalid_argument>([] { clAccelResampler::make(1, 2, 0, 0, 3, 256, std::vector<long long>(2, 1ll << 56)); }));
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    printf("accel host ok\n");
    return 0;
}
