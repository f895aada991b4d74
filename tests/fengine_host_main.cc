// Stand-alone program for tests/test_fengine_host.py: the device-free entry points of clFEngine under -fsanitize=address,undefined, no
// device and nothing loaded into python.  It links the built C ABI library and calls mi355_fengine_plan (sizes, every refusal, NULL
// output pointers), mi355_fengine_create with a NULL context (every argument is checked before the context is touched, and no handle
// comes back), the NULL-handle forms of the other entry points, and -- through host/lib/clFEngine_impl.cc compiled into the program --
// the argument errors of gr::clenabled::clFEngine::make, which are thrown before a context is asked for.
#include <clenabled/clenabled.h>
#include <mi355_clenabled.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, mi355_last_error()); \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

struct Bad {
    int S, npol, F, P, shift;
    const char *msg;
};

template <class E, class Fn> static bool throws(Fn fn)
{
    try {
        fn();
    } catch (const E &) {
        return true;
    } catch (...) {
        return false;
    }
    return false;
}

int main()
{
    using gr::clenabled::clFEngine;
    // sizes
    const int shapes[][4] = {{3, 1, 16, 1}, {2, 2, 64, 1}, {1, 2, 4096, 8}, {5, 2, 256, 4}, {2, 2, 48, 3}, {3, 1, 1000, 2}, {64, 2, 1024, 17}};
    for (const auto &s : shapes)
        for (long long n : {0ll, 1ll, 7ll, 1ll << 20}) {
            long long fb = -1, hi = -1, ni = -1;
            CHECK(mi355_fengine_plan(s[0], s[1], s[2], s[3], 0, n, &fb, &hi, &ni) == MI355_OK);
            CHECK(fb == 2ll * s[0] * s[2] * s[1] && hi == (long long)(s[3] - 1) * s[2] && ni == (n == 0 ? 0 : (n + s[3] - 1) * s[2]));
        }
    CHECK(mi355_fengine_plan(4, 1, 16, 1, 0, 5, nullptr, nullptr, nullptr) == MI355_OK);
    // refusals: from _plan, and from _create before the (NULL, then invalid) context is touched
    const Bad bad[] = {
        {4, 0, 16, 1, 0, "npol must be 1 or 2"},          {4, 3, 16, 1, 0, "npol must be 1 or 2"},
        {0, 1, 16, 1, 0, "num_inputs must be 1 .. 4096"}, {4097, 1, 16, 1, 0, "num_inputs must be 1 .. 4096"},
        {4, 1, 1, 1, 0, "num_channels must be >= 2"},     {4, 1, -3, 1, 0, "num_channels must be >= 2"},
        {4, 1, 16, 0, 0, "taps_per_channel must be 1 .. 1024"}, {4, 1, 16, 1025, 0, "taps_per_channel must be 1 .. 1024"},
        {4, 1, 16, 1, 2, "shift must be 0 or 1"},         {4, 1, 15, 1, 1, "shift needs an even num_channels"},
    };
    for (const Bad &b : bad) {
        long long fb = -1, hi = -1, ni = -1;
        CHECK(mi355_fengine_plan(b.S, b.npol, b.F, b.P, b.shift, 4, &fb, &hi, &ni) == MI355_ERR_INVALID_ARG);
        CHECK(fb == 0 && hi == 0 && ni == 0);
        CHECK(std::string(mi355_last_error()) == std::string("invalid argument: ") + b.msg);
        for (mi355_ctx *ctx : {(mi355_ctx *)nullptr, (mi355_ctx *)0xDEAD0000}) {
            mi355_fengine *h = (mi355_fengine *)1;
            CHECK(mi355_fengine_create(ctx, b.S, b.npol, b.F, b.P, nullptr, b.shift, nullptr, &h) == MI355_ERR_INVALID_ARG && h == nullptr);
            CHECK(std::string(mi355_last_error()) == std::string("invalid argument: ") + b.msg);
        }
    }
    {
        // everything in order but the context; taps and gains given: they are not read before the context is looked at
        std::vector<float> taps(4 * 64, 0.5f), gains(8 * 64, 2.f);
        mi355_fengine *h = (mi355_fengine *)1;
        CHECK(mi355_fengine_create(nullptr, 4, 2, 64, 4, taps.data(), 1, gains.data(), &h) == MI355_ERR_INVALID_ARG && h == nullptr);
        CHECK(std::string(mi355_last_error()) == "invalid argument: NULL context");
        CHECK(mi355_fengine_create(nullptr, 4, 2, 64, 4, nullptr, 1, nullptr, nullptr) == MI355_ERR_INVALID_ARG);
        CHECK(mi355_fengine_plan(4, 1, 16, 1, 0, -1, nullptr, nullptr, nullptr) == MI355_ERR_INVALID_ARG);
        CHECK(mi355_fengine_plan(1, 1, (1 << 24) + 2, 1, 0, 1, nullptr, nullptr, nullptr) == MI355_ERR_UNSUPPORTED);   // clFFT refuses the length
        CHECK(mi355_fengine_plan(4096, 2, 1 << 16, 1, 0, 1, nullptr, nullptr, nullptr) == MI355_ERR_UNSUPPORTED);      // a gain table above 1 GiB
        CHECK(mi355_fengine_plan(1, 1, 4096, 1, 0, 1ll << 61, nullptr, nullptr, nullptr) == MI355_ERR_UNSUPPORTED);    // items past 2^62
    }
    // NULL handles
    CHECK(mi355_fengine_set_gains(nullptr, nullptr) == MI355_ERR_INVALID_ARG && mi355_fengine_set_input_gain(nullptr, 0, nullptr) == MI355_ERR_INVALID_ARG);
    CHECK(mi355_fengine_get_gains(nullptr, nullptr, 0) == MI355_ERR_INVALID_ARG && mi355_fengine_get_clips(nullptr, nullptr, 0) == MI355_ERR_INVALID_ARG);
    CHECK(mi355_fengine_set_generic(nullptr, 1) == MI355_ERR_INVALID_ARG && mi355_fengine_frame_bytes(nullptr) == MI355_ERR_INVALID_ARG);
    CHECK(mi355_fengine_history_items(nullptr) == MI355_ERR_INVALID_ARG && mi355_fengine_destroy(nullptr) == MI355_OK);
    CHECK(mi355_fengine_work(nullptr, 1, nullptr, nullptr) == MI355_ERR_INVALID_ARG && mi355_fengine_work_dev(nullptr, 1, nullptr, nullptr, nullptr) == MI355_ERR_INVALID_ARG);
    CHECK(std::strcmp(mi355_fengine_route(nullptr), "") == 0);
    // the block class: argument errors come before a context (device 99 is never looked for)
    CHECK(throws<std::invalid_argument>([] { clFEngine::make(1, 2, 0, 99, 3, 4, 16); }));
    CHECK(throws<std::invalid_argument>([] { clFEngine::make(1, 2, 0, 99, 2, 4, 15, {}, 1, true); }));
    CHECK(throws<std::invalid_argument>([] { clFEngine::make(1, 2, 0, 99, 2, 4, 16, std::vector<float>(17, 1.f), 1); }));
    CHECK(throws<std::invalid_argument>([] { clFEngine::make(1, 2, 0, 99, 2, 4, 16, {}, 2, false, std::vector<float>(5, 1.f)); }));
    CHECK(throws<std::runtime_error>([] { clFEngine::make(1, 2, 0, 99, 1, 1, 1 << 24, {}, 1, false, std::vector<float>()); }) ||
          throws<std::invalid_argument>([] { clFEngine::make(1, 2, 0, 99, 1, 1, 1 << 24); }));  // an item of 2^25 bytes is legal; a context on device 99 is not
    if (g_fail) return 1;
    printf("fengine host ok\n");
    return 0;
}
