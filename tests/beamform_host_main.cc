// Stand-alone program around host/lib/clBeamformer_impl.cc for tests/test_beamform_host.py: the block class over a STUB of the C ABI,
// no device.  The stub's mi355_beamform_work reads every input byte the contract names (nunits * frames_per_unit * frame_bytes) and
// writes every output byte (nunits * out_bytes_per_unit) -- the test hands it heap buffers of exactly that size, so under
// -fsanitize=address,undefined a work() that passes a frame too few or the wrong unit count is caught -- and records what it was handed.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <vector>

struct mi355_beamform {
    int mode, npol, S, F, B, Ti, stokes, generic;
    long long calls, last_units;
    std::vector<int8_t> w;
};

static int stub_plan(int mode, int npol, int S, int F, int B, int Ti, int stokes, long long *fb, int *fpu, long long *ob)
{
    if ((mode != 0 && mode != 1) || (npol != 1 && npol != 2) || S < 1 || S > 512 || F < 1 || B < 1 || B > 1024 || Ti < 1 || Ti > 4096 ||
        (mode == 0 && Ti != 1) || (stokes && (mode != 1 || npol != 2))) {
        g_err = "invalid argument: stub plan";
        return MI355_ERR_INVALID_ARG;
    }
    if (fb) *fb = 2ll * S * F * npol;
    if (fpu) *fpu = Ti;
    if (ob) *ob = mode == 0 ? 8ll * B * F * npol : 4ll * B * F * (stokes ? 1 : npol);
    return MI355_OK;
}

extern "C" {
int mi355_beamform_plan(int mode, int npol, int S, int F, int B, int Ti, int stokes, long long *fb, int *fpu, long long *ob)
{
    return stub_plan(mode, npol, S, F, B, Ti, stokes, fb, fpu, ob);
}
int mi355_beamform_create(mi355_ctx *ctx, int mode, int npol, int S, int F, int B, int Ti, int stokes, const void *weights, mi355_beamform **out)
{
    if (!ctx || !out || stub_plan(mode, npol, S, F, B, Ti, stokes, nullptr, nullptr, nullptr)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    const size_t n = (size_t)2 * F * npol * B * S;
    const int8_t *w = (const int8_t *)weights;
    for (size_t i = 0; w && i < n; i++)
        if (w[i] == -128) { g_err = "invalid argument: stub weight"; return MI355_ERR_INVALID_ARG; }
    *out = new mi355_beamform{mode, npol, S, F, B, Ti, stokes, 0, 0, 0, w ? std::vector<int8_t>(w, w + n) : std::vector<int8_t>(n, 0)};
    g_live_handles++;
    return MI355_OK;
}
int mi355_beamform_destroy(mi355_beamform *h) { if (h) g_live_handles--; delete h; return MI355_OK; }
int mi355_beamform_set_weights(mi355_beamform *h, const void *weights)
{
    const int8_t *w = (const int8_t *)weights;
    for (size_t i = 0; i < h->w.size(); i++)
        if (w[i] == -128) { g_err = "invalid argument: stub weight"; return MI355_ERR_INVALID_ARG; }
    h->w.assign(w, w + h->w.size());
    return MI355_OK;
}
int mi355_beamform_set_beam_weights(mi355_beamform *h, int beam, const void *w_beam)
{
    if (beam < 0 || beam >= h->B) { g_err = "invalid argument: stub beam"; return MI355_ERR_INVALID_ARG; }
    const size_t per = (size_t)2 * h->S;
    for (int c = 0; c < h->F * h->npol; c++) memcpy(h->w.data() + ((size_t)c * h->B + beam) * per, (const int8_t *)w_beam + (size_t)c * per, per);
    return MI355_OK;
}
int mi355_beamform_get_weights(const mi355_beamform *h, void *out, long long cap)
{
    if (cap < (long long)h->w.size()) { g_err = "invalid argument: stub cap"; return MI355_ERR_INVALID_ARG; }
    memcpy(out, h->w.data(), h->w.size());
    return MI355_OK;
}
int mi355_beamform_set_generic(mi355_beamform *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_beamform_route(const mi355_beamform *h) { return h->generic ? "generic stub" : "mfma stub"; }
int mi355_beamform_work(mi355_beamform *h, long long nunits, const void *in, void *out)
{
    long long fb = 0, ob = 0;
    stub_plan(h->mode, h->npol, h->S, h->F, h->B, h->Ti, h->stokes, &fb, nullptr, &ob);
    const int8_t *x = (const int8_t *)in;
    int sum = 0;
    for (long long i = 0; i < nunits * h->Ti * fb; i++) sum += x[i];  // every byte the contract reads
    unsigned char *y = (unsigned char *)out;
    for (long long i = 0; i < nunits * ob; i++) y[i] = (unsigned char)(h->calls + 1 + 0 * sum);
    h->calls++;
    h->last_units = nunits;
    return MI355_OK;
}
}

using gr::clenabled::clBeamformer;

// one work() call on exact-size heap buffers; returns what work() returned, or -1 when a byte of the output is not the stub's
static int call(clBeamformer &bf, int n, int call_no)
{
    const size_t in_bytes = (size_t)n * bf.decimation() * (size_t)bf.input_signature()->sizeof_stream_item(0);
    const size_t out_bytes = (size_t)n * (size_t)bf.output_signature()->sizeof_stream_item(0);
    std::vector<int8_t> x(in_bytes, -128);
    std::vector<unsigned char> y(out_bytes, 0xEE);
    gr_vector_const_void_star in = {x.data()};
    gr_vector_void_star out = {y.data()};
    const int got = bf.work(n, in, out);
    for (unsigned char v : y)
        if (v != (unsigned char)call_no) return -1;
    return got;
}

static int run(int mode, int npol, int S, int F, int B, int Ti, bool stokes)
{
    const size_t nw = (size_t)2 * F * npol * B * S;
    std::vector<int8_t> w(nw);
    for (size_t i = 0; i < nw; i++) w[i] = (int8_t)((int)(i % 255) - 127);
    auto bf = clBeamformer::make(1, 2, 0, 0, mode, npol, S, F, B, Ti, stokes, w);
    const long long fb = 2ll * S * F * npol, ob = mode == 0 ? 8ll * B * F * npol : 4ll * B * F * (stokes ? 1 : npol);
    // io signature, item sizes, decimation
    CHECK(bf->input_signature()->min_streams() == 1 && bf->input_signature()->max_streams() == 1);
    CHECK(bf->output_signature()->min_streams() == 1 && bf->output_signature()->max_streams() == 1);
    CHECK(bf->input_signature()->sizeof_stream_item(0) == (int)fb && bf->output_signature()->sizeof_stream_item(0) == (int)ob);
    CHECK(bf->frame_bytes() == fb && bf->out_bytes_per_unit() == ob && bf->num_beams() == B);
    CHECK((int)bf->decimation() == (mode == 0 ? 1 : Ti));
    if (mode == 0) CHECK(ob == (long long)sizeof(gr_complex) * B * F * npol);
    CHECK(bf->route() == "mfma stub" && bf->weights() == w);
    // what work() hands the library: n units, n * decimation frames
    int calls = 0;
    for (int n : {1, 2, 7, 33}) CHECK(call(*bf, n, ++calls) == n);
    bf->set_generic(true);
    CHECK(bf->route() == "generic stub");
    // set_weights: the size is checked by the block, the values by the library; a refused update keeps the old set
    std::vector<int8_t> w2(nw, 5);
    bf->set_weights(w2);
    CHECK(bf->weights() == w2);
    for (size_t bad : {(size_t)0, nw - 1, nw + 1, 2 * nw})
        CHECK(throws<std::invalid_argument>([&] { bf->set_weights(std::vector<int8_t>(bad, 1)); }) && bf->weights() == w2);
    std::vector<int8_t> w3(nw, 1);
    w3[nw / 2] = -128;
    CHECK(throws<std::invalid_argument>([&] { bf->set_weights(w3); }) && bf->weights() == w2);
    // set_beam_weights: [f][p][s], one beam of every (f, p)
    const size_t nb = (size_t)2 * F * npol * S;
    std::vector<int8_t> wb(nb, -7);
    bf->set_beam_weights(B - 1, wb);
    const std::vector<int8_t> w4 = bf->weights();
    for (int c = 0; c < F * npol; c++)
        for (int b = 0; b < B; b++)
            for (int i = 0; i < 2 * S; i++) CHECK(w4[((size_t)c * B + b) * 2 * S + i] == (b == B - 1 ? -7 : 5));
    for (size_t bad : {(size_t)0, nb - 1, nb + 1, nw}) {
        if (bad == nb) continue;
        CHECK(throws<std::invalid_argument>([&] { bf->set_beam_weights(0, std::vector<int8_t>(bad, 1)); }) && bf->weights() == w4);
    }
    CHECK(throws<std::invalid_argument>([&] { bf->set_beam_weights(B, wb); }));
    CHECK(call(*bf, 5, ++calls) == 5);
    // no weights at make(): all zero
    auto z = clBeamformer::make(1, 2, 0, 0, mode, npol, S, F, B, Ti, stokes);
    CHECK(z->weights() == std::vector<int8_t>(nw, 0));
    return 0;
}

int main()
{
    for (auto s : {std::vector<int>{0, 1, 4, 8, 1, 1, 0}, {0, 2, 20, 5, 3, 1, 0}, {1, 1, 16, 8, 16, 64, 0}, {1, 2, 64, 8, 5, 32, 1}, {1, 2, 3, 1, 2, 1, 0}}) {
        const int rc = run(s[0], s[1], s[2], s[3], s[4], s[5], s[6] != 0);
        if (rc) return rc;
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // argument errors throw std::invalid_argument before any device work (device 99 does not exist); a missing device is a runtime error
    const std::vector<std::vector<int>> bad = {{2, 1, 4, 8, 2, 1, 0}, {0, 3, 4, 8, 2, 1, 0}, {0, 1, 0, 8, 2, 1, 0},   {0, 1, 513, 8, 2, 1, 0},
                                               {0, 1, 4, 0, 2, 1, 0}, {0, 1, 4, 8, 0, 1, 0}, {0, 1, 4, 8, 1025, 1, 0}, {1, 1, 4, 8, 2, 4097, 0},
                                               {0, 1, 4, 8, 2, 2, 0}, {1, 1, 4, 8, 2, 4, 1}, {0, 2, 4, 8, 2, 1, 1}};
    for (const auto &s : bad)
        CHECK(throws<std::invalid_argument>([&] { clBeamformer::make(1, 2, 0, 99, s[0], s[1], s[2], s[3], s[4], s[5], s[6] != 0); }));
    // a weight vector of the wrong size, before the device is looked for
    CHECK(throws<std::invalid_argument>([] { clBeamformer::make(1, 2, 0, 99, 0, 1, 4, 8, 2, 1, false, std::vector<int8_t>(7, 0)); }));
    // refused by the library: the context is given back
    CHECK(throws<std::invalid_argument>([] { clBeamformer::make(1, 2, 0, 0, 0, 1, 4, 8, 2, 1, false, std::vector<int8_t>(2 * 8 * 2 * 4, -128)); }) &&
          g_live_ctx == 0);
    CHECK(throws<std::runtime_error>([] { clBeamformer::make(1, 2, 0, 99, 0, 1, 4, 8, 2); }, "no such device"));
    printf("beamform host ok\n");
    return 0;
}
