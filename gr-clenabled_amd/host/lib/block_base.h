// What every block unit of host/lib/ shares (internal, header-only: each unit still compiles alone): the log sink, the two error checks,
// the owners of the context and of the library handle, "create or throw", the stream-item check and flat().  BlockBase stands where
// "public GRCLBase" was (include/clenabled/GRCLBase.h:77-141).
#pragma once
#include <clenabled/gr_compat.h>
#include <mi355_clenabled.h>

#include <cstdio>
#include <initializer_list>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace gr {
namespace clenabled {

// The library's diagnostics (mi355_set_log_callback) go where the reference's go: GNU Radio's logger (GR_LOG_INFO / GR_LOG_ERROR,
// lib/clXEngine_impl.cc:107,137,257).  Stand-alone build: stderr, one "clenabled :level: text" line each, like the logger's format.
inline void log_sink(void *, int level, const char *message)
{
#ifdef MI355_WITH_GNURADIO
    // (configure_default_loggers + the GR_LOG_* macros exist in 3.9's log4cpp logger and in 3.10's spdlog one alike)
    static gr::logger_ptr logger, debug_logger;
    static const bool configured = gr::configure_default_loggers(logger, debug_logger, "clenabled");
    (void)configured;
    const std::string text(message);
    switch (level) {
    case MI355_LOG_DEBUG: GR_LOG_DEBUG(debug_logger, text); break;
    case MI355_LOG_INFO: GR_LOG_INFO(logger, text); break;
    case MI355_LOG_WARN: GR_LOG_WARN(logger, text); break;
    default: GR_LOG_ERROR(logger, text); break;
    }
#else
    static const char *const names[] = {"debug", "info", "warning", "error"};
    fprintf(stderr, "clenabled :%s: %s\n", names[level < 0 ? 0 : level > 3 ? 3 : level], message);
#endif
}

inline std::string failure(int rc, const char *what) { return std::string(what) + ": " + mi355_strerror(rc) + ": " + mi355_last_error(); }

// The two error checks; which one a block uses is part of its contract.  Every error code is negative: a positive return is a count
// or a flag (mi355_xcorr_td_poll), never an error.
inline void chk_runtime(int rc, const char *what)
{
    if (rc < 0) throw std::runtime_error(failure(rc, what));
}
inline void chk_arg(int rc, const char *what)
{
    if (rc == MI355_ERR_INVALID_ARG) throw std::invalid_argument(std::string(what) + ": " + mi355_last_error());
    chk_runtime(rc, what);
}

// "create or throw" for the return code of mi355_xxx_create (the reference prints and exit()s, lib/GRCLBase.cpp:239-257): the owners
// below release what exists while the exception unwinds.  Some blocks (those of clenabled_impl.cc among them) report a refused
// argument as a runtime error as well.
enum class ArgIs { invalid_argument, runtime_error };
inline void created(int rc, const char *fn, ArgIs arg = ArgIs::invalid_argument)
{
    if (rc == MI355_ERR_INVALID_ARG && arg == ArgIs::invalid_argument) throw std::invalid_argument(failure(rc, fn));
    if (rc) throw std::runtime_error(failure(rc, fn));
}

inline void check_stream_item(const char *block, std::initializer_list<long long> bytes)
{
    for (long long b : bytes)
        if (b > 0x7fffffffll) throw std::invalid_argument(std::string(block) + ": a stream item of 2 GiB or more");
}

// real taps: the real parts, and an imaginary part that is not zero is refused
inline std::vector<float> flat(const std::vector<gr_complex> &taps, bool complex_taps, const char *block)
{
    std::vector<float> t;
    for (const gr_complex &v : taps) {
        t.push_back(v.real());
        if (complex_taps) t.push_back(v.imag());
        else if (v.imag() != 0.0f) throw std::invalid_argument(std::string(block) + ": complex taps for a block made with real taps");
    }
    return t;
}

// the five make() arguments of every block; open() may come after the block's own argument checks
class Context {
    mi355_ctx *d_p = nullptr;

public:
    Context() {}
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ~Context()
    {
        if (d_p) mi355_ctx_destroy(d_p);
    }
    void open(int openCLPlatformType, int devSelector, int platformId, int devId, bool setDebug, void (*chk)(int, const char *) = chk_runtime)
    {
        static std::once_flag once;  // (one per process: an inline function's static)
        std::call_once(once, [] { mi355_set_log_callback(&log_sink, nullptr); });
        chk(mi355_ctx_create(openCLPlatformType, devSelector, platformId, devId, setDebug ? 1 : 0, &d_p), "mi355_ctx_create");
    }
    operator mi355_ctx *() const { return d_p; }
};

// a library handle and its mi355_xxx_destroy: empty until mi355_xxx_create has written through adopt()
template <class T, int (*Destroy)(T *)>
class Handle {
    T *d_p = nullptr;

public:
    Handle() {}
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    ~Handle() { reset(); }
    T **adopt() { return &d_p; }
    void reset()
    {
        if (d_p) Destroy(d_p);
        d_p = nullptr;
    }
    operator T *() const { return d_p; }
};

template <class T, int (*Destroy)(T *)>
class BlockBase {
protected:
    Context d_ctx;  // declared first: the handle goes before the context does
    Handle<T, Destroy> d_h;
};

}  // namespace clenabled
}  // namespace gr
