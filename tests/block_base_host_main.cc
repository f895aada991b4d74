// Stand-alone program around host/lib/block_base.h for tests/test_block_base_host.py: the base of the block units over the stub context
// of host_stub.h and a toy handle, no device.  The error checks' types and exact texts, what is alive after a failed create and after a
// constructor that throws behind a successful one, the log sink installed once, the handle destroyed before its context.
#include "host_stub.h"
#include "block_base.h"

#include <new>
#include <vector>

struct mi355_toy { int arg; };
static int g_ctx_alive_at_handle_destroy = -1;

extern "C" {
int mi355_toy_create(mi355_ctx *ctx, int arg, mi355_toy **out)
{
    *out = nullptr;
    if (!ctx || arg < 0) { g_err = "stub create"; return MI355_ERR_INVALID_ARG; }
    if (arg == 0) { g_err = "stub memory"; return MI355_ERR_NOMEM; }
    *out = new mi355_toy{arg};
    g_live_handles++;
    return MI355_OK;
}
int mi355_toy_destroy(mi355_toy *h)
{
    g_ctx_alive_at_handle_destroy = g_live_ctx;
    g_live_handles--;
    delete h;
    return MI355_OK;
}
}

using namespace gr::clenabled;

// a block as the units write it: context, handle, then something that may throw (set_history, a message port, a vector)
struct Toy : BlockBase<mi355_toy, mi355_toy_destroy> {
    Toy(int dev, int arg, bool arg_errors, bool throw_after)
    {
        d_ctx.open(1, 2, 0, dev, false, arg_errors ? chk_arg : chk_runtime);
        created(mi355_toy_create(d_ctx, arg, d_h.adopt()), "mi355_toy_create", arg_errors ? ArgIs::invalid_argument : ArgIs::runtime_error);
        if (throw_after) throw std::bad_alloc();
    }
    int arg() const { return ((mi355_toy *)d_h)->arg; }
};

// the pattern the units had before: raw pointers and a destructor, which a throwing constructor never reaches
struct Before {
    mi355_ctx *d_ctx = nullptr;
    mi355_toy *d_h = nullptr;
    Before(mi355_ctx **ctx, mi355_toy **h)
    {
        mi355_ctx_create(1, 2, 0, 0, 0, &d_ctx);
        mi355_toy_create(d_ctx, 1, &d_h);
        *ctx = d_ctx;
        *h = d_h;
        throw std::bad_alloc();
    }
    ~Before()
    {
        mi355_toy_destroy(d_h);
        mi355_ctx_destroy(d_ctx);
    }
};

// what() of the E that f() throws; "" when it throws nothing or something else
template <class E, class F>
std::string what_of(F &&f)
{
    try { f(); } catch (const E &e) { return e.what(); } catch (...) { }
    return "";
}

int main()
{
    // the two checks: nothing for MI355_OK or a count, the type and the exact text otherwise
    g_err = "E";
    chk_runtime(MI355_OK, "w");
    chk_arg(MI355_OK, "w");
    chk_runtime(1, "w");
    chk_arg(1, "w");
    CHECK(what_of<std::runtime_error>([] { chk_runtime(MI355_ERR_INVALID_ARG, "w"); }) == "w: invalid argument: E");
    CHECK(what_of<std::runtime_error>([] { chk_runtime(MI355_ERR_NOMEM, "w"); }) == "w: error: E");
    CHECK(what_of<std::invalid_argument>([] { chk_arg(MI355_ERR_INVALID_ARG, "w"); }) == "w: E");
    CHECK(what_of<std::runtime_error>([] { chk_arg(MI355_ERR_NOMEM, "w"); }) == "w: error: E");
    CHECK(g_sink_installs == 0);  // nothing before the first context

    // a block that works: one context, one handle, the handle goes first
    {
        Toy a(0, 5, true, false), b(0, 6, false, false);
        CHECK(a.arg() == 5 && b.arg() == 6 && g_live_ctx == 2 && g_live_handles == 2);
    }
    CHECK(g_live_ctx == 0 && g_live_handles == 0 && g_ctx_alive_at_handle_destroy == 1);

    // "create or throw" on a refused create: type and text of each flavour, and the context is given back
    CHECK(what_of<std::invalid_argument>([] { Toy(0, -1, true, false); }) == "mi355_toy_create: invalid argument: stub create");
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    CHECK(what_of<std::runtime_error>([] { Toy(0, -1, false, false); }) == "mi355_toy_create: invalid argument: stub create");
    CHECK(what_of<std::runtime_error>([] { Toy(0, 0, true, false); }) == "mi355_toy_create: error: stub memory");
    CHECK(what_of<std::runtime_error>([] { Toy(0, 0, false, false); }) == "mi355_toy_create: error: stub memory");
    CHECK(g_live_ctx == 0 && g_live_handles == 0);
    // no device: a runtime error from either check, nothing alive
    for (bool arg_errors : {true, false})
        CHECK(what_of<std::runtime_error>([&] { Toy(99, 1, arg_errors, false); }) == "mi355_ctx_create: no device: no such device");
    CHECK(g_live_ctx == 0 && g_live_handles == 0);

    // a constructor that throws behind a successful create releases both, handle first ...
    g_ctx_alive_at_handle_destroy = -1;
    CHECK(throws<std::bad_alloc>([] { Toy(0, 1, true, true); }));
    CHECK(g_live_ctx == 0 && g_live_handles == 0 && g_ctx_alive_at_handle_destroy == 1);
    // ... which the raw pointers and the destructor of before did not
    mi355_ctx *ctx = nullptr;
    mi355_toy *h = nullptr;
    CHECK(throws<std::bad_alloc>([&] { Before(&ctx, &h); }));
    CHECK(g_live_ctx == 1 && g_live_handles == 1);
    mi355_toy_destroy(h);
    mi355_ctx_destroy(ctx);

    // the sink: installed once for all of the blocks above, and it is the block layer's
    CHECK(g_sink_installs == 1 && g_sink == &log_sink);

    // Handle: empty until adopted, reset() destroys once
    {
        Context c;
        c.open(1, 2, 0, 0, false);
        Handle<mi355_toy, mi355_toy_destroy> t;
        CHECK((mi355_toy *)t == nullptr);
        t.reset();
        CHECK(g_live_handles == 0);
        CHECK(mi355_toy_create(c, 3, t.adopt()) == MI355_OK && g_live_handles == 1);
        t.reset();
        CHECK(g_live_handles == 0 && (mi355_toy *)t == nullptr);
    }
    CHECK(g_live_ctx == 0 && g_sink_installs == 1);

    // the stream-item check and flat()
    check_stream_item("clToy", {0, 0x7fffffffll});
    CHECK(what_of<std::invalid_argument>([] { check_stream_item("clToy", {1, 0x80000000ll}); }) == "clToy: a stream item of 2 GiB or more");
    const std::vector<gr_complex> taps = {gr_complex(1.f, 0.f), gr_complex(2.f, 0.f)};
    CHECK(flat(taps, false, "clToy") == (std::vector<float>{1.f, 2.f}) && flat(taps, true, "clToy") == (std::vector<float>{1.f, 0.f, 2.f, 0.f}));
    CHECK(what_of<std::invalid_argument>([] { flat({gr_complex(1.f, 0.5f)}, false, "clToy"); }) == "clToy: complex taps for a block made with real taps");
    printf("block_base host ok\n");
    return 0;
}
