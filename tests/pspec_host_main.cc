// Stand-alone program around host/lib/clPowerSpectrum_impl.cc for tests/test_pspec_host.py: the block class over a STUB of the C ABI, no
// device.  The stub's mi355_pspec_work reads every input item and writes every output float the contract names -- from heap buffers of
// exactly that size, so under -fsanitize=address,undefined a general_work() that offers the library one item too few or asks for one
// spectrum too many is caught -- and returns P[s][b] = s + b / 1024 so that the caller can tell which spectra were made.  The caller
// declares what it offers (set_offered): a consume of more than that throws, as GNU Radio's buffer accounting would break.
#include <clenabled/clenabled.h>
#include "host_stub.h"

#include <algorithm>
#include <vector>

struct mi355_pspec { int N, K, H; float scale; int generic; long long calls; std::vector<float> window; };

extern "C" {
int mi355_pspec_plan(int N, int K, int H, long long S, long long *nin, long long *nout)
{
    if (N < 1 || K < 1 || H < 1 || S < 0) { g_err = "invalid argument: stub"; return MI355_ERR_INVALID_ARG; }
    if (N == 1) { g_err = "fft size 1 unsupported"; return MI355_ERR_UNSUPPORTED; }
    if (nin) *nin = S == 0 ? 0 : (S * K - 1) * H + N;
    if (nout) *nout = S * N;
    return MI355_OK;
}
int mi355_pspec_create(mi355_ctx *ctx, int N, const float *window, int window_len, int K, int H, int, int, float scale, mi355_pspec **out)
{
    if (!ctx || !out || (window_len != 0 && window_len != N)) { g_err = "invalid argument: stub create"; return MI355_ERR_INVALID_ARG; }
    *out = new mi355_pspec{N, K, H, scale, 0, 0, std::vector<float>(window, window + window_len)};
    return MI355_OK;
}
int mi355_pspec_destroy(mi355_pspec *h) { delete h; return MI355_OK; }
int mi355_pspec_set_scale(mi355_pspec *h, float scale) { h->scale = scale; return MI355_OK; }
int mi355_pspec_set_window(mi355_pspec *h, const float *window, int window_len)
{
    if (window_len != 0 && window_len != h->N) { g_err = "invalid argument: stub window"; return MI355_ERR_INVALID_ARG; }
    h->window.assign(window, window + window_len);
    return MI355_OK;
}
int mi355_pspec_set_generic(mi355_pspec *h, int on) { h->generic = on; return MI355_OK; }
const char *mi355_pspec_route(const mi355_pspec *h) { return h->generic ? "generic stub" : "fused stub"; }
int mi355_pspec_work(mi355_pspec *h, long long S, const void *in, void *out)
{
    long long nin = 0, nout = 0;
    mi355_pspec_plan(h->N, h->K, h->H, S, &nin, &nout);
    const float *x = (const float *)in;
    float sum = 0.f;
    for (long long i = 0; i < 2 * nin; i++) sum += x[i];  // every item the contract reads
    float *y = (float *)out;
    for (long long s = 0; s < S; s++)
        for (int b = 0; b < h->N; b++) y[s * h->N + b] = (float)(h->calls * 100 + s) + (float)b / 1024.f + 0.f * sum;
    h->calls++;
    return MI355_OK;
}
}

using gr::clenabled::clPowerSpectrum;

static int run(int N, int K, int H)
{
    auto ps = clPowerSpectrum::make(1, 2, 0, 0, N, K, std::vector<float>((size_t)N, 0.5f), H == N ? 0 : H, true, false, 2.0f);
    CHECK(ps->fft_size() == N && ps->navg() == K && ps->hop() == H && ps->route() == "fused stub");
    CHECK((int)ps->history() == (N > H ? N - H : 0) + 1);
    ps->set_generic(true);
    CHECK(ps->route() == "generic stub");
    ps->set_scale(3.0f);
    ps->set_window(std::vector<float>());
    ps->set_window(std::vector<float>((size_t)N, 1.0f));
    CHECK(throws<std::invalid_argument>([&] { ps->set_window(std::vector<float>((size_t)N + 1, 1.0f)); }));
    gr_vector_int req(1, -1);
    ps->forecast(3, req);
    CHECK(req[0] == std::max((3 * K - 1) * H + N, 3 * K * H));
    // exact-size heap buffers: what S spectra need, offered with up to a whole spectrum less one item on top (never enough for S + 1)
    for (int S : {0, 1, 4}) {
        for (int extra : {0, 1, K * H - 1}) {
            if (extra >= K * H) continue;
            // what S spectra need: the items the library reads and, with hop > fft_size, the skipped items the block consumes
            const long need = S == 0 ? 0 : std::max(((long)S * K - 1) * H + N, (long)S * K * H);
            const long have = need == 0 ? (extra < N ? extra : N - 1) : need + extra;
            std::vector<gr_complex> x((size_t)have, gr_complex(1.f, -1.f));
            for (int room : {S, S + 2}) {
                std::vector<float> y((size_t)room * N, -1.f);
                gr_vector_int ni(1, (int)have);
                gr_vector_const_void_star in = {x.data()};
                gr_vector_void_star out = {y.data()};
                ps->reset_consumed();
                ps->set_offered(ni);
                const int got = ps->general_work(room, ni, in, out);
                CHECK(got == S && ps->nitems_consumed(0) == (long)S * K * H);
                for (int s = 0; s < S; s++) CHECK((int)y[(size_t)s * N] % 100 == s);
                for (size_t i = (size_t)S * N; i < y.size(); i++) CHECK(y[i] == -1.f);
            }
            // less room than input: the room decides
            if (S >= 2) {
                std::vector<float> y((size_t)(S - 1) * N, -1.f);
                gr_vector_int ni(1, (int)have);
                gr_vector_const_void_star in = {x.data()};
                gr_vector_void_star out = {y.data()};
                ps->reset_consumed();
                ps->set_offered(ni);
                CHECK(ps->general_work(S - 1, ni, in, out) == S - 1 && ps->nitems_consumed(0) == (long)(S - 1) * K * H);
            }
        }
    }
    if (H > N) {
        const long have = ((long)K - 1) * H + N;  // every frame of one spectrum, not yet the items skipped after the last
        std::vector<gr_complex> x((size_t)have, gr_complex(1.f, -1.f));
        std::vector<float> y((size_t)N, -1.f);
        gr_vector_int ni(1, (int)have);
        gr_vector_const_void_star in = {x.data()};
        gr_vector_void_star out = {y.data()};
        ps->reset_consumed();
        ps->set_offered(ni);
        CHECK(ps->general_work(1, ni, in, out) == 0 && ps->nitems_consumed(0) == 0 && y[0] == -1.f);
    }
    // the model itself refuses a consume of more than was offered
    {
        ps->reset_consumed();
        ps->set_offered(gr_vector_int(1, K * H - 1));
        CHECK(throws<std::logic_error>([&] { ps->consume_each(K * H); }));
        ps->reset_consumed();
    }
    return 0;
}

int main()
{
    for (auto shape : {std::vector<int>{64, 4, 64}, {64, 3, 16}, {16, 5, 100}, {100, 1, 1}}) {
        const int rc = run(shape[0], shape[1], shape[2]);
        if (rc) return rc;
    }
    // argument errors throw std::invalid_argument before any device work; what clFFT refuses and a missing device are runtime errors
    for (auto bad : {std::vector<int>{0, 4, 4}, {64, 0, 64}, {64, 4, -1}})
        CHECK(throws<std::invalid_argument>([&] { clPowerSpectrum::make(1, 2, 0, 99, bad[0], bad[1], std::vector<float>(), bad[2]); }));
    CHECK(throws<std::invalid_argument>([] { clPowerSpectrum::make(1, 2, 0, 0, 64, 4, std::vector<float>(63, 1.f)); }));
    CHECK(throws<std::runtime_error>([] { clPowerSpectrum::make(1, 2, 0, 0, 1, 4); }, "fft size 1"));
    CHECK(throws<std::runtime_error>([] { clPowerSpectrum::make(1, 2, 0, 99, 64, 4); }, "no such device"));
    printf("pspec host ok\n");
    return 0;
}
