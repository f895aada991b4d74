// Stand-alone program around HostPipe, mi355_pageable_run, DevBuf and DevWorkspace (csrc/common.h, csrc/hostpipe.hip) for
// tests/test_hostpipe_host.py: the two drivers behind every block's host-pointer work(), the staging pipeline first and the piece
// loop of the pageable paths after it, then the stream-ordered workspace of clFFT, clPowerSpectrum and clFEngine, over SYNCHRONOUS HOST STUBS of the dozen HIP runtime calls they make, no device.  "Device"
// and pinned buffers are heap blocks of exactly the size ensure() asked for and the caller's buffers are heap blocks of exactly the
// size describe() names, so under -fsanitize=address,undefined a copy of one byte too many is caught.  The "kernel" is a host
// function: output byte j of chunk ci = input byte j (xor the second input's) xor key(ci).  Every stubbed call is logged, and the
// order the driver promises is read off that log.
#include "common.h"

#include <cstdarg>
#include <string>

// ---- the log -------------------------------------------------------------------------------------------------------------------
enum Kind { EV_RECORD, EV_SYNC, COPY_IN, COPY_OUT, H2D, D2H, STREAM_SYNC, DIRECT_SYNC, LAUNCH, DELIVER, FAIL, DEV_MALLOC, DEV_FREE, STREAM_WAIT };
struct Entry { Kind kind; int slot; size_t arg; };
static std::vector<Entry> g_log;
static HostPipe *g_pipe = nullptr;  // nullptr: the pageable driver and DevBuf are under test, and hipMalloc / hipFree are logged too
static int g_memcpy_calls = 0, g_memcpy_fail_at = -1;  // the g_memcpy_fail_at-th hipMemcpyAsync fails, once
static int g_malloc_calls = 0, g_malloc_fail_at = -1;  // the same for hipMalloc
static int g_sync_calls = 0, g_sync_fail_at = -1;      // and for hipStreamSynchronize
static bool g_capturing = false;                       // what hipStreamIsCapturing answers
static std::string g_err;

static int slot_of_event(hipEvent_t e)
{
    for (int s = 0; g_pipe && s < HostPipe::kSlots; s++)
        if (g_pipe->done[s] == e) return s;
    return -1;
}
// slot whose pinned / device buffer `p` is (any input or the output), -1: none of the staging
static int slot_of(void *const (*in)[HostPipe::MAXIN], void *const *out, const void *p)
{
    for (int s = 0; s < HostPipe::kSlots; s++) {
        for (int i = 0; i < HostPipe::MAXIN; i++)
            if (in[s][i] && in[s][i] == p) return s;
        if (out[s] && out[s] == p) return s;
    }
    return -1;
}
static void log_host_copy(void *dst, const void *src, size_t bytes)
{
    if (!bytes) return;
    const int to = slot_of(g_pipe->h_in, g_pipe->h_out, dst), from = slot_of(g_pipe->h_in, g_pipe->h_out, src);
    if (to >= 0) g_log.push_back({COPY_IN, to, bytes});
    else g_log.push_back({COPY_OUT, from, bytes});
    memcpy(dst, src, bytes);
}

// ---- the project's own helpers the driver calls (runtime.hip has them; that unit holds device code) ----------------------------
void mi355_set_error(const char *fmt, ...)
{
    char line[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof(line), fmt, ap);
    va_end(ap);
    g_err = line;
}
void mi355_log(const mi355_ctx *, int, const char *, ...) {}
void mi355_copy_notes(const mi355_ctx *) {}
void mi355_copy2(void *dst0, const void *src0, size_t bytes0, void *dst1, const void *src1, size_t bytes1)
{
    log_host_copy(dst0, src0, bytes0);
    log_host_copy(dst1, src1, bytes1);
}
void mi355_copy(void *dst, const void *src, size_t bytes) { log_host_copy(dst, src, bytes); }
hipError_t mi355_direct_sync(hipStream_t)
{
    g_log.push_back({DIRECT_SYNC, -1, 0});
    return hipSuccess;
}

// ---- the HIP runtime, as synchronous host stubs --------------------------------------------------------------------------------
static int g_live_allocs = 0, g_live_events = 0;
extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
hipError_t hipMalloc(void **p, size_t bytes)
{
    if (g_malloc_calls++ == g_malloc_fail_at) {
        g_log.push_back({FAIL, -1, bytes});
        return hipErrorOutOfMemory;
    }
    if (!g_pipe) g_log.push_back({DEV_MALLOC, -1, bytes});
    *p = malloc(bytes);
    g_live_allocs++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *p)
{
    if (!g_pipe) g_log.push_back({DEV_FREE, -1, 0});
    if (p) g_live_allocs--;
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return hipMalloc(p, bytes); }
hipError_t hipHostFree(void *p) { return hipFree(p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(1); g_live_events++; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); g_live_events--; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t st)
{
    g_log.push_back({EV_RECORD, slot_of_event(e), (size_t)st});
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    g_log.push_back({EV_SYNC, slot_of_event(e), 0});
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t st, hipEvent_t, unsigned int)
{
    g_log.push_back({STREAM_WAIT, -1, (size_t)st});
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *status)
{
    *status = g_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st)
{
    g_log.push_back({STREAM_SYNC, -1, (size_t)st});
    return g_sync_calls++ == g_sync_fail_at ? hipErrorUnknown : hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    if (g_memcpy_calls++ == g_memcpy_fail_at) {
        g_log.push_back({FAIL, -1, 0});
        return hipErrorInvalidValue;
    }
    const bool in = kind == hipMemcpyHostToDevice;
    g_log.push_back({in ? H2D : D2H, g_pipe ? slot_of(g_pipe->d_in, g_pipe->d_out, in ? dst : src) : -1, (size_t)st});
    memcpy(dst, src, bytes);
    return hipSuccess;
}
}

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stderr, "line %d: %s\n", __LINE__, #c);           \
            return 1;                                                 \
        }                                                             \
    } while (0)

// ---- one call through the pipeline ---------------------------------------------------------------------------------------------
static const size_t kChunk = 1000, kRagged = 667;  // bytes of a chunk and of the last one
static unsigned char key(size_t ci) { return (unsigned char)(ci * 37 + 11); }
static size_t chunk_bytes(size_t ci, size_t nchunks) { return ci + 1 == nchunks ? kRagged : kChunk; }

struct Call {
    size_t nchunks = 1;
    int nin = 1;
    HostPipe::Plan plan;
    bool zero_out = false;        // every chunk describes out_bytes 0
    long fail_launch_at = -1;     // launch of this chunk returns MI355_ERR_UNSUPPORTED
    bool custom = false;          // deliver through a callback
    // results
    int rc = 0;
    std::vector<unsigned char> out, want;  // the caller's output buffer (filled with 0xEE before the call) and what a whole call computes
    std::vector<size_t> delivered;  // chunk numbers the callback saw
    bool deliver_saw_right_bytes = true;
};

static int run_call(mi355_ctx *ctx, Call &c)
{
    HostPipe pipe;
    g_pipe = &pipe;
    g_log.clear();
    g_memcpy_calls = 0;
    CHECK(pipe.init(ctx) == MI355_OK);
    const size_t total = (c.nchunks - 1) * kChunk + kRagged;
    // exact-size heap buffers: one byte read or written past them is ASan's to report
    unsigned char *a = (unsigned char *)malloc(total), *b = (unsigned char *)malloc(total);
    for (size_t j = 0; j < total; j++) { a[j] = (unsigned char)(j * 7 + 3); b[j] = (unsigned char)(j * 13 + 5); }
    c.out.assign(total, 0xEE);
    const size_t cap[2] = {kChunk, kChunk};
    CHECK(pipe.ensure(c.nin, cap, kChunk, c.plan.nslots) == MI355_OK);
    auto describe = [&](size_t ci) {
        HostPipe::Chunk ch;
        ch.src[0] = a + ci * kChunk;
        ch.in_bytes[0] = chunk_bytes(ci, c.nchunks);
        if (c.nin == 2) { ch.src[1] = b + ci * kChunk; ch.in_bytes[1] = ch.in_bytes[0]; }
        ch.dst = c.custom ? nullptr : c.out.data() + ci * kChunk;
        ch.out_bytes = c.zero_out ? 0 : ch.in_bytes[0];
        return ch;
    };
    auto launch = [&](size_t ci, void *const *in, void *out, hipStream_t st) -> int {
        if ((long)ci == c.fail_launch_at) {
            g_log.push_back({FAIL, -1, ci});
            return MI355_ERR_UNSUPPORTED;
        }
        g_log.push_back({LAUNCH, -1, (size_t)st});
        const unsigned char *x = (const unsigned char *)in[0], *y = (const unsigned char *)in[1];
        for (size_t j = 0; j < chunk_bytes(ci, c.nchunks); j++) ((unsigned char *)out)[j] = x[j] ^ (c.nin == 2 ? y[j] : 0) ^ key(ci);
        return MI355_OK;
    };
    if (c.custom)
        c.rc = pipe.run(c.nchunks, c.plan, describe, launch, [&](size_t ci, const void *pinned) {
            g_log.push_back({DELIVER, -1, ci});
            c.delivered.push_back(ci);
            const unsigned char *p = (const unsigned char *)pinned;
            for (size_t j = 0; j < chunk_bytes(ci, c.nchunks); j++) {
                if (p[j] != (unsigned char)(a[ci * kChunk + j] ^ (c.nin == 2 ? b[ci * kChunk + j] : 0) ^ key(ci))) c.deliver_saw_right_bytes = false;
                c.out[ci * kChunk + j] = p[j];
            }
        });
    else c.rc = pipe.run(c.nchunks, c.plan, describe, launch);
    c.want.resize(total);
    for (size_t j = 0; j < total; j++) c.want[j] = (unsigned char)(a[j] ^ (c.nin == 2 ? b[j] : 0) ^ key(j / kChunk));
    free(a);
    free(b);
    pipe.release();
    g_pipe = nullptr;
    return 0;
}

// chunk ci of the caller's output holds the kernel's result / still holds the fill it had before the call
static bool in_place(const Call &c, size_t ci) { return memcmp(&c.out[ci * kChunk], &c.want[ci * kChunk], chunk_bytes(ci, c.nchunks)) == 0; }
static bool untouched(const Call &c, size_t ci)
{
    for (size_t j = 0; j < chunk_bytes(ci, c.nchunks); j++)
        if (c.out[ci * kChunk + j] != 0xEE) return false;
    return true;
}
static size_t count(Kind k)
{
    size_t n = 0;
    for (const Entry &e : g_log) n += e.kind == k;
    return n;
}

// The order the driver promises, read off the log.  A slot is in flight from its first DMA until it is waited for: by a synchronise
// of its event, if the event was recorded behind the slot's last DMA, or by a synchronise of the stream the DMA went to.  (For a copy
// into h_in[s] after the slot's first chunk that means: the last event call on slot s before it is a synchronise, not a record.)
//   - no host copy touches the staging of a slot in flight: neither the next input in nor a result out;
//   - after a failure nothing is copied, launched or delivered any more, only waited for;
//   - when the call returns, failed or not, no slot is in flight.
static int check_order()
{
    bool in_flight[HostPipe::kSlots] = {}, covered[HostPipe::kSlots] = {}, failed = false;
    size_t stream[HostPipe::kSlots] = {};
    for (const Entry &e : g_log) {
        if (failed) CHECK(e.kind == EV_SYNC || e.kind == STREAM_SYNC);
        switch (e.kind) {
        case H2D: case D2H:
            CHECK(e.slot >= 0);
            in_flight[e.slot] = true;
            covered[e.slot] = false;
            stream[e.slot] = e.arg;
            break;
        case EV_RECORD:
            CHECK(e.slot >= 0 && e.arg == stream[e.slot]);
            covered[e.slot] = true;
            break;
        case EV_SYNC:
            CHECK(e.slot >= 0);
            if (covered[e.slot]) in_flight[e.slot] = false;
            break;
        case STREAM_SYNC:
            for (int s = 0; s < HostPipe::kSlots; s++)
                if (stream[s] == e.arg) in_flight[s] = false;
            break;
        case COPY_IN: case COPY_OUT: CHECK(e.slot >= 0 && !in_flight[e.slot]); break;
        case FAIL: failed = true; break;
        default: break;
        }
    }
    for (int s = 0; s < HostPipe::kSlots; s++) CHECK(!in_flight[s]);
    return 0;
}

// ---- one call through the piece loop of the pageable paths --------------------------------------------------------------------
// A unit is kUnit bytes of each input and of output 0 and kUnit / 2 bytes of output 1.  Input a carries kHist bytes of history in
// front, which every piece sends again (as the synthesizer and clFEngine do); input b carries none.  The "kernel":
//   out0[j] = a[j] ^ a[j + kHist] ^ b[j],   out1[j] = b[2 j] ^ 0x5A   -- no piece number in it: any split gives the same bytes.
// The caller's arrays and the DevBufs are heap blocks of exactly the size needed, so ASan sees a copy of one byte too many.
static const size_t kUnit = 100, kHist = 30;

struct PCall {
    long long total = 1, want = 1;
    long fail_launch_at = -1;  // the launch of this piece returns MI355_ERR_UNSUPPORTED
    // results
    int rc = 0;
    long long per = 0;         // units per piece as clamped
    std::vector<long long> firsts, counts;
    std::vector<unsigned char> out0, out1, want0, want1;
};

static int run_pcall(mi355_ctx *ctx, PCall &c)
{
    g_log.clear();
    g_memcpy_calls = g_sync_calls = 0;
    const size_t total = (size_t)c.total;
    unsigned char *a = (unsigned char *)malloc(total * kUnit + kHist), *b = (unsigned char *)malloc(total * kUnit);
    for (size_t j = 0; j < total * kUnit + kHist; j++) a[j] = (unsigned char)(j * 7 + 3);
    for (size_t j = 0; j < total * kUnit; j++) b[j] = (unsigned char)(j * 13 + 5);
    unsigned char *o0 = (unsigned char *)malloc(total * kUnit), *o1 = (unsigned char *)malloc(total * kUnit / 2);
    memset(o0, 0xEE, total * kUnit);
    memset(o1, 0xEE, total * kUnit / 2);
    c.per = mi355_piece_units(c.want, c.total);
    DevBuf da, db, d0, d1;
    const size_t per = (size_t)c.per;
    CHECK(da.reserve(per * kUnit + kHist) == MI355_OK && db.reserve(per * kUnit) == MI355_OK);
    CHECK(d0.reserve(per * kUnit) == MI355_OK && d1.reserve(per * kUnit / 2) == MI355_OK);
    g_log.clear();
    long npiece = 0;
    c.rc = mi355_pageable_run(ctx, c.total, c.want, [&](long long first, long long n, hipStream_t st) -> int {
        c.firsts.push_back(first);
        c.counts.push_back(n);
        const size_t f = (size_t)first * kUnit, bytes = (size_t)n * kUnit;
        MI355_HIP(hipMemcpyAsync(da.get(), a + f, bytes + kHist, hipMemcpyHostToDevice, st));
        MI355_HIP(hipMemcpyAsync(db.get(), b + f, bytes, hipMemcpyHostToDevice, st));
        if (npiece++ == c.fail_launch_at) {
            g_log.push_back({FAIL, -1, (size_t)first});
            return MI355_ERR_UNSUPPORTED;
        }
        g_log.push_back({LAUNCH, -1, (size_t)st});
        const unsigned char *x = (const unsigned char *)da.get(), *y = (const unsigned char *)db.get();
        for (size_t j = 0; j < bytes; j++) ((unsigned char *)d0.get())[j] = x[j] ^ x[j + kHist] ^ y[j];
        for (size_t j = 0; j < bytes / 2; j++) ((unsigned char *)d1.get())[j] = y[2 * j] ^ 0x5A;
        MI355_HIP(hipMemcpyAsync(o0 + f, d0.get(), bytes, hipMemcpyDeviceToHost, st));
        MI355_HIP(hipMemcpyAsync(o1 + f / 2, d1.get(), bytes / 2, hipMemcpyDeviceToHost, st));
        return MI355_OK;
    });
    c.out0.assign(o0, o0 + total * kUnit);
    c.out1.assign(o1, o1 + total * kUnit / 2);
    c.want0.resize(total * kUnit);
    c.want1.resize(total * kUnit / 2);
    for (size_t j = 0; j < total * kUnit; j++) c.want0[j] = a[j] ^ a[j + kHist] ^ b[j];
    for (size_t j = 0; j < total * kUnit / 2; j++) c.want1[j] = b[2 * j] ^ 0x5A;
    const std::vector<Entry> log = g_log;  // of the run alone
    for (DevBuf *d : {&da, &db, &d0, &d1}) d->release();
    g_log = log;
    for (unsigned char *p : {a, b, o0, o1}) free(p);
    return 0;
}

// units [u0, u1) of output `which` hold the kernel's result / still hold the fill they had before the call
static bool p_done(const PCall &c, int which, long long u0, long long u1)
{
    const size_t w = which ? kUnit / 2 : kUnit;
    return memcmp((which ? c.out1 : c.out0).data() + u0 * w, (which ? c.want1 : c.want0).data() + u0 * w, (size_t)(u1 - u0) * w) == 0;
}
static bool p_untouched(const PCall &c, int which, long long u0, long long u1)
{
    const size_t w = which ? kUnit / 2 : kUnit;
    for (size_t j = (size_t)u0 * w; j < (size_t)u1 * w; j++)
        if ((which ? c.out1 : c.out0)[j] != 0xEE) return false;
    return true;
}
static bool log_is(std::initializer_list<Kind> kinds, size_t from)
{
    size_t i = from;
    for (Kind k : kinds)
        if (i >= g_log.size() || g_log[i++].kind != k) return false;
    return true;
}

static int pageable_cases(mi355_ctx *ctx)
{
    const long long kPer = 4, kLast = 3;  // units of a full piece and of the ragged last one
    // 1 to 5 pieces: every output byte, and per piece H2D H2D LAUNCH D2H D2H STREAM_SYNC on ctx->stream[0], nothing else
    for (long long np = 1; np <= 5; np++) {
        PCall c;
        c.total = (np - 1) * kPer + kLast;
        c.want = kPer;
        CHECK(run_pcall(ctx, c) == 0);
        CHECK(c.rc == MI355_OK && c.out0 == c.want0 && c.out1 == c.want1);
        CHECK((long long)c.firsts.size() == np && g_log.size() == (size_t)np * 6);
        for (long long i = 0; i < np; i++) {
            CHECK(c.firsts[i] == i * c.per && c.counts[i] == (i + 1 == np ? kLast : kPer));
            CHECK(log_is({H2D, H2D, LAUNCH, D2H, D2H, STREAM_SYNC}, (size_t)i * 6));
        }
        for (const Entry &e : g_log) CHECK(e.kind == LAUNCH || e.kind == H2D || e.kind == D2H || e.kind == STREAM_SYNC);
        for (const Entry &e : g_log) CHECK((hipStream_t)e.arg == ctx->stream[0]);
    }
    // a total smaller than the wanted piece is one piece of `total` units; a wanted piece of 0 is held to one unit, so it is one piece
    // of `total` units for total = 1 and `total` pieces of one unit otherwise (min(max(want, 1), total))
    {
        PCall c;
        c.total = 3;
        c.want = 1000;
        CHECK(run_pcall(ctx, c) == 0);
        CHECK(c.rc == MI355_OK && c.per == 3 && c.firsts.size() == 1 && c.counts[0] == 3 && c.out0 == c.want0 && c.out1 == c.want1);
        for (long long total : {1ll, 3ll})
            for (long long want : {0ll, -5ll}) {
                PCall z;
                z.total = total;
                z.want = want;
                CHECK(run_pcall(ctx, z) == 0);
                CHECK(z.rc == MI355_OK && z.per == 1 && (long long)z.firsts.size() == total && z.out0 == z.want0 && z.out1 == z.want1);
                for (long long n : z.counts) CHECK(n == 1);
            }
        CHECK(mi355_piece_units((size_t)0, (size_t)7) == 1 && mi355_piece_units((size_t)9, (size_t)7) == 7 && mi355_piece_units(5, 7) == 5);
    }
    // a launch that fails in piece k of 4: its code comes back, the stream is waited for behind the failure, nothing follows that wait,
    // and no output byte of a piece >= k is touched
    for (long k = 0; k < 4; k++) {
        PCall c;
        c.total = 3 * kPer + kLast;
        c.want = kPer;
        c.fail_launch_at = k;
        CHECK(run_pcall(ctx, c) == 0);
        CHECK(c.rc == MI355_ERR_UNSUPPORTED && (long)c.firsts.size() == k + 1);
        CHECK(g_log.size() == (size_t)k * 6 + 4 && log_is({H2D, H2D, FAIL, STREAM_SYNC}, (size_t)k * 6));
        for (int which = 0; which <= 1; which++) CHECK(p_done(c, which, 0, k * kPer) && p_untouched(c, which, k * kPer, c.total));
    }
    // the n-th hipMemcpyAsync failing, every n of a four-piece call (four copies per piece): MI355_ERR_HIP and the same drain.  The
    // outputs of the pieces behind the failed one are untouched, and so is every output of the failed piece that was not queued
    // before the failure (output 0 was when the copy of output 1 fails).
    for (int n = 0; n < 16; n++) {
        PCall c;
        c.total = 3 * kPer + kLast;
        c.want = kPer;
        g_memcpy_fail_at = n;
        CHECK(run_pcall(ctx, c) == 0);
        g_memcpy_fail_at = -1;
        const long long k = n / 4, u0 = k * kPer, u1 = k == 3 ? c.total : u0 + kPer;
        CHECK(c.rc == MI355_ERR_HIP && g_err.find("hipMemcpyAsync") != std::string::npos && (long long)c.firsts.size() == k + 1);
        CHECK(count(FAIL) == 1 && g_log.size() >= 2 && g_log[g_log.size() - 2].kind == FAIL && g_log.back().kind == STREAM_SYNC);
        CHECK(g_log.size() == (size_t)k * 6 + (n % 4 < 2 ? n % 4 : n % 4 + 1) + 2);
        for (int which = 0; which <= 1; which++) CHECK(p_done(c, which, 0, u0) && p_untouched(c, which, u1, c.total));
        CHECK(n % 4 == 3 ? p_done(c, 0, u0, u1) : p_untouched(c, 0, u0, u1));
        CHECK(p_untouched(c, 1, u0, u1));
    }
    // the wait behind piece 1 failing: one more wait, MI355_ERR_HIP, no third piece
    {
        PCall c;
        c.total = 3 * kPer + kLast;
        c.want = kPer;
        g_sync_fail_at = 1;
        CHECK(run_pcall(ctx, c) == 0);
        g_sync_fail_at = -1;
        CHECK(c.rc == MI355_ERR_HIP && g_err.find("hipStreamSynchronize") != std::string::npos && c.firsts.size() == 2);
        CHECK(g_log.size() == 13 && log_is({H2D, H2D, LAUNCH, D2H, D2H, STREAM_SYNC, STREAM_SYNC}, 6));
        for (int which = 0; which <= 1; which++) CHECK(p_untouched(c, which, 2 * kPer, c.total));
    }
    return 0;
}

static int devbuf_cases()
{
    DevBuf d;
    CHECK(d.get() == nullptr && d.bytes() == 0);
    g_log.clear();
    CHECK(d.reserve(0) == MI355_OK && d.get() == nullptr && g_log.empty());
    CHECK(d.reserve(100) == MI355_OK && d.get() != nullptr && d.bytes() == 100);
    CHECK(g_log.size() == 1 && g_log[0].kind == DEV_MALLOC && g_log[0].arg == 100);
    memset(d.get(), 1, 100);  // exactly that many bytes are there
    // a smaller or equal reserve keeps the block
    void *const p = d.get();
    CHECK(d.reserve(100) == MI355_OK && d.reserve(7) == MI355_OK && d.get() == p && d.bytes() == 100 && g_log.size() == 1);
    // a larger one frees first, then allocates
    CHECK(d.reserve(101) == MI355_OK && d.bytes() == 101 && g_live_allocs == 1);
    CHECK(g_log.size() == 3 && g_log[1].kind == DEV_FREE && g_log[2].kind == DEV_MALLOC && g_log[2].arg == 101);
    memset(d.get(), 2, 101);
    // a failed allocation leaves the buffer empty (the old block is gone), and the next reserve works
    g_malloc_fail_at = g_malloc_calls;
    CHECK(d.reserve(500) == MI355_ERR_HIP && d.get() == nullptr && d.bytes() == 0 && g_live_allocs == 0);
    CHECK(g_err.find("hipMalloc") != std::string::npos);
    g_malloc_fail_at = -1;
    CHECK(d.reserve(50) == MI355_OK && d.get() != nullptr && d.bytes() == 50 && g_live_allocs == 1);
    memset(d.get(), 3, 50);
    d.release();
    CHECK(d.get() == nullptr && d.bytes() == 0 && g_live_allocs == 0);
    d.release();  // twice is harmless
    CHECK(d.reserve(10) == MI355_OK && d.bytes() == 10);
    d.release();
    CHECK(g_live_allocs == 0);
    return 0;
}

// DevWorkspace: what acquire / release / wait / destroy promise, read off the log (no pipe: hipMalloc / hipFree are logged)
static int workspace_cases()
{
    const hipStream_t s1 = (hipStream_t)0x10, s2 = (hipStream_t)0x20;
    const int allocs0 = g_live_allocs, events0 = g_live_events;
    DevWorkspace w;
    g_log.clear();
    // the host wait with no user yet is a no-op
    CHECK(w.wait() == MI355_OK && g_log.empty() && w.get() == nullptr && w.bytes() == 0);
    // first acquire: no wait of either kind, the allocation alone; release records on the caller's stream and remembers it
    CHECK(w.acquire(100, s1) == MI355_OK && w.get() != nullptr && w.bytes() == 100);
    CHECK(g_log.size() == 1 && g_log[0].kind == DEV_MALLOC && g_log[0].arg == 100 && g_live_events == events0 + 1);
    memset(w.get(), 1, 100);
    CHECK(w.release(s1) == MI355_OK && g_log.size() == 2 && g_log[1].kind == EV_RECORD && (hipStream_t)g_log[1].arg == s1 && w.last_stream() == s1);
    // the same stream again: no wait
    g_log.clear();
    CHECK(w.acquire(100, s1) == MI355_OK && g_log.empty() && w.release(s1) == MI355_OK);
    // another stream: one stream-wait on the event, of that stream, before anything else
    g_log.clear();
    CHECK(w.acquire(50, s2) == MI355_OK && g_log.size() == 1 && g_log[0].kind == STREAM_WAIT && (hipStream_t)g_log[0].arg == s2);
    CHECK(w.release(s2) == MI355_OK && w.last_stream() == s2 && w.bytes() == 100);
    // grow while used: the host waits for the event before the old block is freed and the new one allocated
    g_log.clear();
    CHECK(w.acquire(200, s1) == MI355_OK && g_log.size() == 4 && log_is({STREAM_WAIT, EV_SYNC, DEV_FREE, DEV_MALLOC}, 0) && w.bytes() == 200);
    memset(w.get(), 2, 200);
    CHECK(w.release(s1) == MI355_OK);
    g_log.clear();
    CHECK(w.acquire(201, s1) == MI355_OK && g_log.size() == 3 && log_is({EV_SYNC, DEV_FREE, DEV_MALLOC}, 0) && w.release(s1) == MI355_OK);
    // the host wait for the last user
    g_log.clear();
    CHECK(w.wait() == MI355_OK && g_log.size() == 1 && g_log[0].kind == EV_SYNC);
    // release under capture: no event record, and the remembered stream stays
    g_capturing = true;
    g_log.clear();
    CHECK(w.acquire(10, s2) == MI355_OK && w.release(s2) == MI355_OK);
    g_capturing = false;
    CHECK(count(EV_RECORD) == 0 && w.last_stream() == s1 && g_log.size() == 1 && g_log[0].kind == STREAM_WAIT);
    // a failed hipMalloc leaves the workspace empty, and the next acquire allocates
    g_malloc_fail_at = g_malloc_calls;
    g_log.clear();
    CHECK(w.acquire(1000, s1) == MI355_ERR_HIP && w.get() == nullptr && w.bytes() == 0 && g_live_allocs == allocs0);
    CHECK(log_is({EV_SYNC, DEV_FREE, FAIL}, 0) && g_err.find("hipMalloc") != std::string::npos);
    g_malloc_fail_at = -1;
    g_log.clear();
    CHECK(w.acquire(30, s1) == MI355_OK && w.get() != nullptr && w.bytes() == 30 && count(DEV_MALLOC) == 1 && count(DEV_FREE) == 0);
    memset(w.get(), 3, 30);
    CHECK(w.release(s1) == MI355_OK);
    // grow while never used: no wait
    {
        DevWorkspace v;
        g_log.clear();
        CHECK(v.acquire(10, s1) == MI355_OK && v.acquire(20, s2) == MI355_OK && v.bytes() == 20);
        CHECK(g_log.size() == 3 && log_is({DEV_MALLOC, DEV_FREE, DEV_MALLOC}, 0));
        v.destroy();
    }
    // after destroy the allocation and the event are gone; twice is harmless, and the object starts over
    w.destroy();
    CHECK(w.get() == nullptr && w.bytes() == 0 && g_live_allocs == allocs0 && g_live_events == events0);
    w.destroy();
    g_log.clear();
    CHECK(w.acquire(5, s2) == MI355_OK && g_log.size() == 1 && g_log[0].kind == DEV_MALLOC && w.release(s2) == MI355_OK);
    w.destroy();
    CHECK(g_live_allocs == allocs0 && g_live_events == events0);
    return 0;
}

int main()
{
    mi355_ctx ctx;
    ctx.stream[0] = (hipStream_t)0x10;
    ctx.stream[1] = (hipStream_t)0x20;

    // placement and reuse: every output byte lands where describe() said, slots are waited for before they are refilled, and each
    // chunk runs on the stream of its slot
    const size_t shapes[][2] = {{1, 4}, {4, 4}, {5, 4}, {6, 4}, {9, 4}, {3, 1}, {3, 2}};  // chunks, slots
    for (const auto &sh : shapes)
        for (int nin = 1; nin <= 2; nin++)
            for (int one_stream = 0; one_stream <= 1; one_stream++) {
                Call c;
                c.nchunks = sh[0];
                c.nin = nin;
                c.plan.nslots = (int)sh[1];
                c.plan.one_stream = one_stream != 0;
                CHECK(run_call(&ctx, c) == 0);
                CHECK(c.rc == MI355_OK && c.out == c.want);
                CHECK(check_order() == 0);
                CHECK(count(COPY_IN) == c.nchunks * nin && count(H2D) == c.nchunks * nin && count(D2H) == c.nchunks);
                CHECK(count(LAUNCH) == c.nchunks && count(COPY_OUT) == c.nchunks && count(DIRECT_SYNC) == 0);
                // one wait per chunk: on the slot's event, or with a single slot on the stream (no event is recorded then)
                const size_t with_events = sh[1] > 1 ? c.nchunks : 0;
                CHECK(count(EV_RECORD) == with_events && count(EV_SYNC) == with_events && count(STREAM_SYNC) == c.nchunks - with_events);
                size_t ci = 0;
                for (const Entry &e : g_log)
                    if (e.kind == D2H) {
                        const int s = (int)(ci++ % sh[1]);
                        CHECK(e.slot == s && (hipStream_t)e.arg == ctx.stream[one_stream ? 0 : (s & 1)]);
                    }
            }

    // the direct path: the kernel works on the pinned staging, chunk after chunk in slot 0; no DMA, no event
    for (size_t nchunks : {(size_t)1, (size_t)3})
        for (int nin = 1; nin <= 2; nin++) {
            Call c;
            c.nchunks = nchunks;
            c.nin = nin;
            c.plan.direct = true;
            CHECK(run_call(&ctx, c) == 0);
            CHECK(c.rc == MI355_OK && c.out == c.want);
            CHECK(count(H2D) + count(D2H) + count(EV_RECORD) + count(EV_SYNC) == 0);
            CHECK(count(DIRECT_SYNC) == nchunks && count(LAUNCH) == nchunks && count(COPY_IN) == nchunks * nin && count(COPY_OUT) == nchunks);
            for (const Entry &e : g_log)
                if (e.kind == COPY_IN || e.kind == COPY_OUT) CHECK(e.slot == 0);
        }

    // zero output bytes: nothing comes back and nothing is delivered, and the slots are still recycled behind their events
    {
        Call c;
        c.nchunks = 6;
        c.zero_out = true;
        CHECK(run_call(&ctx, c) == 0);
        CHECK(c.rc == MI355_OK);
        for (size_t ci = 0; ci < c.nchunks; ci++) CHECK(untouched(c, ci));
        CHECK(count(D2H) == 0 && count(COPY_OUT) == 0 && count(LAUNCH) == 6 && count(EV_RECORD) == 6 && count(EV_SYNC) == 6);
        CHECK(check_order() == 0);
    }

    // a launch that fails at the fifth chunk of nine: its code comes back, the slots in flight are drained first, and only what was
    // delivered before the failure (the first 5 - nslots chunks) is in the caller's buffer
    for (int custom = 0; custom <= 1; custom++) {
        Call c;
        c.nchunks = 9;
        c.fail_launch_at = 4;
        c.custom = custom != 0;
        CHECK(run_call(&ctx, c) == 0);
        CHECK(c.rc == MI355_ERR_UNSUPPORTED);
        CHECK(in_place(c, 0));
        for (size_t ci = 1; ci < c.nchunks; ci++) CHECK(untouched(c, ci));
        CHECK(check_order() == 0 && count(FAIL) == 1);
        CHECK(count(EV_SYNC) == 4);  // slot 0 before its reuse, slots 1 2 3 in the drain
    }

    // a runtime call that fails once (the D2H of chunk 5, slot 1): MI355_ERR_HIP, with the same drain
    for (int nslots : {4, 2, 1}) {
        Call c;
        c.nchunks = 9;
        c.plan.nslots = nslots;
        g_memcpy_fail_at = 2 * 5 + 1;
        CHECK(run_call(&ctx, c) == 0);
        g_memcpy_fail_at = -1;
        CHECK(c.rc == MI355_ERR_HIP && g_err.find("hipMemcpyAsync") != std::string::npos);
        for (size_t ci = 0; ci < c.nchunks; ci++) CHECK(ci + nslots <= 5 ? in_place(c, ci) : untouched(c, ci));
        CHECK(check_order() == 0 && count(FAIL) == 1);
    }

    // custom delivery: the callback is handed the pinned output of the right chunk, once per chunk and oldest first
    for (int nslots : {1, 2, 4})
        for (size_t nchunks : {(size_t)1, (size_t)3, (size_t)6, (size_t)9})
            for (int direct = 0; direct <= 1; direct++) {
                Call c;
                c.nchunks = nchunks;
                c.plan.nslots = nslots;
                c.plan.direct = direct != 0;
                c.custom = true;
                CHECK(run_call(&ctx, c) == 0);
                CHECK(c.rc == MI355_OK && c.deliver_saw_right_bytes && c.out == c.want);
                CHECK(c.delivered.size() == nchunks && count(COPY_OUT) == 0);
                for (size_t ci = 0; ci < nchunks; ci++) CHECK(c.delivered[ci] == ci);
                CHECK(check_order() == 0);
            }

    CHECK(g_live_allocs == 0 && g_live_events == 0);

    CHECK(pageable_cases(&ctx) == 0);
    CHECK(devbuf_cases() == 0);
    CHECK(workspace_cases() == 0);
    CHECK(g_live_allocs == 0 && g_live_events == 0);
    printf("hostpipe host ok\n");
    return 0;
}
