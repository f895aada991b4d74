// What the block-stub programs (tests/*_host_main.cc) share: the stub context of the C ABI with its live count, the error text, the log
// callback (recorded, not called), CHECK and throws<>.  Each program adds the stub of its own block's functions.  It holds definitions:
// one translation unit of a program includes it.
#pragma once
#include <mi355_clenabled.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

struct mi355_ctx { int dev; };

std::string g_err;
int g_live_ctx = 0, g_live_handles = 0, g_sink_installs = 0;
mi355_log_fn g_sink = nullptr;

extern "C" {
const char *mi355_strerror(int code) { return code == MI355_ERR_INVALID_ARG ? "invalid argument" : code == MI355_ERR_NO_DEVICE ? "no device" : "error"; }
const char *mi355_last_error(void) { return g_err.c_str(); }
int mi355_set_log_callback(mi355_log_fn fn, void *) { g_sink = fn; g_sink_installs++; return MI355_OK; }
// device 99 does not exist
int mi355_ctx_create(int, int, int, int dev_id, int, mi355_ctx **out)
{
    if (dev_id == 99) { g_err = "no such device"; return MI355_ERR_NO_DEVICE; }
    *out = new mi355_ctx{dev_id};
    g_live_ctx++;
    return MI355_OK;
}
int mi355_ctx_destroy(mi355_ctx *ctx) { delete ctx; g_live_ctx--; return MI355_OK; }
}

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);           \
            return 1;                                                 \
        }                                                             \
    } while (0)

// f() throws an E -- and, with `text`, one whose what() contains it; anything else it throws is a failure too
template <class E, class F>
bool throws(F &&f, const char *text = nullptr)
{
    try { f(); } catch (const E &e) { return !text || strstr(e.what(), text) != nullptr; } catch (...) { }
    return false;
}
