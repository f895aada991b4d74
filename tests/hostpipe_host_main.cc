// Stand-alone program around HostPipe (csrc/common.h, csrc/hostpipe.hip) for tests/test_hostpipe_host.py: the staging pipeline that
// drives every block's host-pointer work(), over SYNCHRONOUS HOST STUBS of the dozen HIP runtime calls it makes, no device.  "Device"
// and pinned buffers are heap blocks of exactly the size ensure() asked for and the caller's buffers are heap blocks of exactly the
// size describe() names, so under -fsanitize=address,undefined a copy of one byte too many is caught.  The "kernel" is a host
// function: output byte j of chunk ci = input byte j (xor the second input's) xor key(ci).  Every stubbed call is logged, and the
// order the driver promises is read off that log.
#include "common.h"

#include <cstdarg>
#include <string>

// ---- the log -------------------------------------------------------------------------------------------------------------------
enum Kind { EV_RECORD, EV_SYNC, COPY_IN, COPY_OUT, H2D, D2H, STREAM_SYNC, DIRECT_SYNC, LAUNCH, DELIVER, FAIL };
struct Entry { Kind kind; int slot; size_t arg; };
static std::vector<Entry> g_log;
static HostPipe *g_pipe = nullptr;
static int g_memcpy_calls = 0, g_memcpy_fail_at = -1;  // the g_memcpy_fail_at-th hipMemcpyAsync fails, once
static std::string g_err;

static int slot_of_event(hipEvent_t e)
{
    for (int s = 0; s < HostPipe::kSlots; s++)
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
hipError_t hipMalloc(void **p, size_t bytes) { *p = malloc(bytes); g_live_allocs++; return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *p) { if (p) g_live_allocs--; free(p); return hipSuccess; }
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
hipError_t hipStreamSynchronize(hipStream_t st)
{
    g_log.push_back({STREAM_SYNC, -1, (size_t)st});
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    if (g_memcpy_calls++ == g_memcpy_fail_at) {
        g_log.push_back({FAIL, -1, 0});
        return hipErrorInvalidValue;
    }
    const bool in = kind == hipMemcpyHostToDevice;
    g_log.push_back({in ? H2D : D2H, slot_of(g_pipe->d_in, g_pipe->d_out, in ? dst : src), (size_t)st});
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
    printf("hostpipe host ok\n");
    return 0;
}
