// Internal helpers shared by the HIP translation units behind mi355_clenabled.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "mi355_clenabled.h"

struct mi355_ctx {
    int device = 0;
    int debug = 0;
    hipStream_t stream[2] = {nullptr, nullptr};  // [0] = compute stream handed out by mi355_ctx_stream
    int num_cus = 0;
    std::mutex lock;
    // table uploads (create / set_taps): their own stream, so that only this stream is waited for -- a hipDeviceSynchronize() here
    // would stall every other block working on the device while one filter is retuned
    hipStream_t upload = nullptr;
    std::mutex upload_lock;
};

// host -> device copy of a table on the context's upload stream, complete (on the device) when it returns; `src` may be freed at once
hipError_t mi355_upload(mi355_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
// device-side fill on the upload stream, complete when it returns
hipError_t mi355_fill(mi355_ctx *ctx, void *dst_dev, int value, size_t bytes);

// A device table that a setter may replace while kernels of earlier work_dev calls still read it: the version in use plus the
// replaced ones that are not known to be idle yet.  Every block with such a table keeps one of these.  The caller holds the
// handle's lock and has set the device.  publish / drop / release are for create, the setters and destroy: they free, and release
// waits, so they are never called on the work path.  Nothing here waits for the device as a whole.
struct mi355_tables {
    // a new version holding `bytes` of `img`, complete on the device when this returns; the one before is retired and the retired
    // versions whose readers have finished are freed.  On failure the version in use stays and the error reads "`what` upload: ..."
    int publish(mi355_ctx *ctx, const void *img, size_t bytes, const char *what);
    void *current() const { return cur.d; }
    // retires the version in use without a successor: current() is NULL until the next publish
    void drop();
    // after the launches of a call that read current(): the version outlives what `st` holds so far.  Records an event, no more.
    int used(hipStream_t st);
    // waits for the readers recorded here (this object's own events only) and frees every version
    void release();
    size_t held() const { return retired.size(); }

private:
    static constexpr int kSlots = 4;
    struct Version {
        void *d = nullptr;
        size_t bytes = 0;
        // readers, one slot per stream; a slot is in use once it has an event.  A fifth stream takes a slot over (see used)
        hipStream_t st[kSlots] = {};
        hipEvent_t ev[kSlots] = {};
        int next = 0;
    };
    Version cur;
    std::vector<Version> retired;
    void reap(bool wait);
};

void mi355_set_error(const char *fmt, ...);
// one diagnostics line to the registered sink (mi355_set_log_callback) or, by default, to stderr; DEBUG / INFO lines are
// dropped unless the context was created with debug != 0 (the reference's setDebug)
void mi355_log(const mi355_ctx *ctx, int level, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

// A switch that is read once per process at launch time says so the first time a non-default value is acted on under a debug context:
// one INFO line, "switch NAME: what runs instead" (how tests/test_switches_once_gpu.py knows that the switch reached the code it names).
#define MI355_SWITCH_NOTE(ctx, name, what)                                                                   \
    do {                                                                                                     \
        static std::atomic<bool> said__{false};                                                              \
        if ((ctx) && (ctx)->debug && !said__.exchange(true)) mi355_log((ctx), MI355_LOG_INFO, "switch %s: %s", name, what); \
    } while (0)

// the same for a switch that is read per call: `cond` (which may call getenv) is only evaluated under a debug context
#define MI355_SWITCH_NOTE_IF(ctx, cond, name, what)                                  \
    do {                                                                             \
        if ((ctx) && (ctx)->debug && (cond)) MI355_SWITCH_NOTE(ctx, name, what);     \
    } while (0)

#define MI355_HIP(call)                                                                  \
    do {                                                                                 \
        hipError_t e__ = (call);                                                         \
        if (e__ != hipSuccess) {                                                         \
            mi355_set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e__)); \
            return MI355_ERR_HIP;                                                        \
        }                                                                                \
    } while (0)

#define MI355_REQUIRE(cond, msg)                         \
    do {                                                 \
        if (!(cond)) {                                   \
            mi355_set_error("invalid argument: %s", msg); \
            return MI355_ERR_INVALID_ARG;                \
        }                                                \
    } while (0)

static inline size_t mi355_dtype_size(int dtype)
{
    switch (dtype) {
    case MI355_DTYPE_COMPLEX: return 8;
    case MI355_DTYPE_FLOAT: return 4;
    case MI355_DTYPE_INT: return 4;
    case MI355_DTYPE_SHORT: return 2;
    case MI355_DTYPE_BYTE: return 2;   // interleaved int8 I,Q (lib/clXEngine_impl.cc:66-68)
    case MI355_DTYPE_PACKEDXY: return 1;
    }
    return 0;
}

// `stream` is a hipStream_t passed through the C ABI as void*; NULL is HIP's
// default (null) stream, which is also torch's default stream.
static inline hipStream_t mi355_pick_stream(mi355_ctx *, void *stream) { return (hipStream_t)stream; }

// compute units of the context's device (256, the MI355X's, where the query gave nothing)
static inline int mi355_cus(const mi355_ctx *ctx) { return ctx->num_cus > 0 ? ctx->num_cus : 256; }

// grid of a grid-stride kernel of 256-thread workgroups over `total` items: one workgroup per 256 items, at most per_cu per CU
static inline unsigned mi355_grid_256(const mi355_ctx *ctx, long long total, int per_cu)
{
    const long long g = (total + 255) / 256, cap = (long long)mi355_cus(ctx) * per_cu;
    return (unsigned)(g > cap ? cap : g < 1 ? 1 : g);
}

// do the pb bytes at p and the qb bytes at q share a byte?
static inline bool mi355_overlap(const void *p, long long pb, const void *q, long long qb)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

// Persistent-kernel grid: k workgroups per CU, k in [kmin, kmax] (all resident).  More resident
// workgroups hide latency better, so kmax is the default; a smaller k is taken only when it divides
// the work units more evenly by more than `tol` (a ragged last round costs up to 1/rounds of the
// run time; latency-bound kernels pass a large tol, the bandwidth-bound FFT a small one).  MI355_WG_PER_CU overrides (tuning aid).
static inline int mi355_balanced_grid(const mi355_ctx *ctx, long long units, int kmin, int kmax, double tol = 0.08)
{
    const int cus = mi355_cus(ctx);
    if (const char *e = getenv("MI355_WG_PER_CU")) {
        const int k = atoi(e);
        if (k > 0) return units < (long long)cus * k ? (units < 1 ? 1 : (int)units) : cus * k;
    }
    if (units <= (long long)cus * kmin) return units < 1 ? 1 : (int)units;
    auto eff = [&](int k) {
        const long long grid = (long long)cus * k, rounds = (units + grid - 1) / grid;
        return (double)units / (double)(rounds * grid);
    };
    int best = kmax;
    for (int k = kmax - 1; k >= kmin; k--)
        if (eff(k) > eff(best) + tol) best = k;
    return cus * best;
}

// ---------------------------------------------------------------------------
// Pinned staging for the host-pointer work() path (HostPipe below): slot s runs H2D -> kernel -> D2H on
// ctx->stream[s & 1], so the copy-in of chunk c+1 overlaps the kernel / copy-out of chunk c (north_star:
// "pinned double-buffered H2D/D2H overlapping compute on HIP streams").
// ---------------------------------------------------------------------------
// Host calls whose buffers are at most this large (a scheduler-sized work() call) skip the H2D / D2H copy submissions: the
// kernel reads and writes the pinned staging buffers across PCIe itself -- one launch and one synchronisation per call
// (8192-item clMathOp.work(): 58 us -> 23 us on MI355X).  MI355_NO_DIRECT=1 disables it.
constexpr size_t kDirectBytes = 512u << 10;
static inline bool mi355_direct_ok(size_t max_buffer_bytes, const mi355_ctx *ctx = nullptr)
{
    static const bool off = getenv("MI355_NO_DIRECT") != nullptr;
    if (off && max_buffer_bytes <= kDirectBytes) MI355_SWITCH_NOTE(ctx, "MI355_NO_DIRECT", "staged copies for a call the direct path would take");
    return !off && max_buffer_bytes <= kDirectBytes;
}
// Completion wait of such a call (one kernel of a few microseconds): poll the stream for a bounded time, then sleep on it.
// The device's scheduling flags are left alone (a process-wide hipDeviceScheduleSpin would make every blocking wait of
// every block in a thread-per-block flowgraph burn a core); MI355_SPIN_US sets the polling window, 0 = always sleep.
hipError_t mi355_direct_sync(hipStream_t st);

// Staging copy of the host path (caller's pageable buffer <-> pinned staging).  One thread moves ~13 GB/s, which bounded the
// large host calls at 1.8 GS/s (PCIe would carry 3x that): copies of 2 MiB and more are split over a small persistent pool
// (MI355_COPY_THREADS, default 7 helpers; 0 = the calling thread alone), streaming stores (MI355_COPY_STREAM=0: plain memcpy).  If the pool is busy with another block's copy the caller just
// copies alone.
void mi355_copy(void *dst, const void *src, size_t bytes);
// says once (MI355_SWITCH_NOTE) which of MI355_COPY_THREADS=0 / MI355_COPY_STREAM=0 these copies run with
void mi355_copy_notes(const mi355_ctx *ctx);
// Staging chunk of a large host call of `total` bytes per buffer: 8 MiB pieces keep both DMA directions busy (40 GB/s each way of
// the 48 this link carries with unbounded transfers); a call of only a few MiB is cut into >= 6 pieces of >= 1 MiB so that its
// copy-in, transfers and copy-out overlap at all (one 8 MiB piece ran them strictly one after the other).  MI355_CHUNK_MB overrides.
static inline size_t mi355_chunk_bytes(size_t total, const mi355_ctx *ctx = nullptr)
{
    static const size_t forced = getenv("MI355_CHUNK_MB") ? (size_t)atoi(getenv("MI355_CHUNK_MB")) << 20 : 0;
    if (ctx && ctx->debug) mi355_copy_notes(ctx);
    if (forced) {
        MI355_SWITCH_NOTE(ctx, "MI355_CHUNK_MB", "forced staging chunk");
        return forced;
    }
    size_t c = total / 6;
    if (c > ((size_t)8 << 20)) c = (size_t)8 << 20;
    if (c < ((size_t)1 << 20)) c = (size_t)1 << 20;
    return c & ~(size_t)4095;
}
// two copies as one job of the pool (a staging slot's copy-out and copy-in side by side); either may be empty
void mi355_copy2(void *dst0, const void *src0, size_t bytes0, void *dst1, const void *src1, size_t bytes1);
// runs fn(arg, part, parts) for part = 0..parts-1 on the pool (part 0 on the caller); false = pool busy or disabled, nothing was run
bool mi355_parallel(void (*fn)(void *, int part, int parts), void *arg);

struct HostPipe {
    static constexpr int MAXIN = 2;
    // Four slots on the context's two streams (slot s runs on stream s & 1).  A slot's cycle is copy-in -> H2D -> kernel -> D2H ->
    // copy-out; with two slots the host copies of one slot and the DMAs of the other took turns (8 MiB per 0.49 ms = 34 GB/s each
    // way on a link that carries 48); with four the DMA queues never run dry.
    static constexpr int kSlots = 4;
    mi355_ctx *ctx = nullptr;
    size_t cap_in[MAXIN] = {0, 0};
    size_t cap_out = 0;
    void *h_in[kSlots][MAXIN] = {};
    void *d_in[kSlots][MAXIN] = {};
    void *h_out[kSlots] = {};
    void *d_out[kSlots] = {};
    hipEvent_t done[kSlots] = {};

    int init(mi355_ctx *c);
    // staging for `nslots` slots (the first nslots; a frame of 32 MiB and more is staged through two slots only)
    int ensure(int nin, const size_t *in_bytes, size_t out_bytes, int nslots = kSlots);
    int slots_ready = 0;
    void release();

    // One chunk of a host call as its block describes it: where the caller's inputs lie (in_bytes 0 = no such input) and where the
    // output goes.  out_bytes 0 = nothing comes back for this chunk; `dst` is not read when run() is given a deliver callback.
    struct Chunk {
        const void *src[MAXIN] = {};
        size_t in_bytes[MAXIN] = {};
        void *dst = nullptr;
        size_t out_bytes = 0;
    };
    // units in part i of `total` units cut `per` at a time (the last part is the ragged one)
    static size_t part(size_t total, size_t per, size_t i) { return total - i * per < per ? total - i * per : per; }
    struct Plan {
        int nslots = kSlots;      // 1: the chunks run strictly one after the other
        bool one_stream = false;  // every chunk on ctx->stream[0] (kernels that share work buffers)
        bool direct = false;      // the kernel works on the pinned staging itself (mi355_direct_ok, decided by the block)
    };
    // The host-pointer work() of a block: chunks 0 .. nchunks-1 through the staging slots, chunk i in slot i % nslots.  The block has
    // called ensure() for its largest chunk and holds its locks; the device is set.
    //   describe(i) -> Chunk
    //   launch(i, void *const *in, void *out, hipStream_t) -> MI355_* code; `in` / `out` are the slot's device buffers (direct: pinned)
    //   deliver(i, const void *pinned_out): for a block whose output is not one contiguous copy; nullptr = copy to Chunk::dst
    // Per chunk: wait for the slot if it is busy, its previous result out beside its next input in (mi355_copy2), H2D per input,
    // launch, D2H, event record.  On any failure the slots in flight are waited for before the code is returned, so no DMA or
    // kernel outlives the call on this staging, and nothing more is delivered.
    template <class Describe, class Launch, class Deliver = std::nullptr_t>
    int run(size_t nchunks, const Plan &plan, Describe &&describe, Launch &&launch, Deliver &&deliver = nullptr);
};

template <class Describe, class Launch, class Deliver>
int HostPipe::run(size_t nchunks, const Plan &plan, Describe &&describe, Launch &&launch, Deliver &&deliver)
{
    constexpr bool custom = !std::is_same<typename std::decay<Deliver>::type, std::nullptr_t>::value;
    auto copy_out = [&](size_t ci, void *dst, const void *pinned, size_t bytes) {
        if (bytes == 0) return;
        if constexpr (custom) deliver(ci, pinned);
        else mi355_copy(dst, pinned, bytes);
    };
    hipStream_t st = ctx->stream[0];
    struct { bool busy; size_t ci; void *dst; size_t bytes; } pend[kSlots] = {};
    const int nslots = plan.nslots < 1 ? 1 : plan.nslots > kSlots ? kSlots : plan.nslots;
    // With one slot nothing else is queued on the stream, so the stream itself is waited for and no event is recorded: the record
    // and the wait for its marker behind the D2H cost a one-transfer call (the channelizer's 80 us) about 9 us.
    const bool events = nslots > 1;
    auto wait = [&](int s) { return events ? hipEventSynchronize(done[s]) : hipStreamSynchronize(ctx->stream[0]); };
    const int rc = [&]() -> int {
        if (plan.direct) {
            for (size_t ci = 0; ci < nchunks; ci++) {
                const Chunk c = describe(ci);
                for (int i = 0; i < MAXIN; i++)
                    if (c.in_bytes[i]) mi355_copy(h_in[0][i], c.src[i], c.in_bytes[i]);
                const int lrc = launch(ci, h_in[0], h_out[0], st);
                if (lrc) return lrc;
                MI355_HIP(mi355_direct_sync(st));
                copy_out(ci, c.dst, h_out[0], c.out_bytes);
            }
            return MI355_OK;
        }
        for (size_t ci = 0; ci < nchunks; ci++) {
            const int s = (int)(ci % nslots);
            st = ctx->stream[plan.one_stream ? 0 : (s & 1)];
            if (pend[s].busy) MI355_HIP(wait(s));  // slot busy with chunk ci - nslots: drain it
            const Chunk c = describe(ci);
            const auto was = pend[s];
            pend[s] = {};
            // the slot's previous result out and its next input in, side by side
            if constexpr (custom) {
                copy_out(was.ci, nullptr, h_out[s], was.bytes);
                mi355_copy(h_in[s][0], c.src[0], c.in_bytes[0]);
            } else mi355_copy2(was.dst, h_out[s], was.bytes, h_in[s][0], c.src[0], c.in_bytes[0]);
            if (c.in_bytes[1]) mi355_copy(h_in[s][1], c.src[1], c.in_bytes[1]);
            for (int i = 0; i < MAXIN; i++)
                if (c.in_bytes[i]) MI355_HIP(hipMemcpyAsync(d_in[s][i], h_in[s][i], c.in_bytes[i], hipMemcpyHostToDevice, st));
            const int lrc = launch(ci, d_in[s], d_out[s], st);
            if (lrc) return lrc;
            if (c.out_bytes) MI355_HIP(hipMemcpyAsync(h_out[s], d_out[s], c.out_bytes, hipMemcpyDeviceToHost, st));
            if (events) MI355_HIP(hipEventRecord(done[s], st));
            pend[s] = {true, ci, c.dst, c.out_bytes};
        }
        for (int q = 0; q < nslots; q++) {
            const int s = (int)((nchunks + q) % nslots);  // oldest slot first
            if (!pend[s].busy) continue;
            MI355_HIP(wait(s));
            pend[s].busy = false;
            copy_out(pend[s].ci, pend[s].dst, h_out[s], pend[s].bytes);
        }
        return MI355_OK;
    }();
    if (rc != MI355_OK) {
        // what the slots still hold is waited for, then what the failed chunk itself had queued on its stream
        for (int s = 0; s < nslots; s++)
            if (pend[s].busy) (void)wait(s);
        (void)hipStreamSynchronize(st);
    }
    return rc;
}

// ---------------------------------------------------------------------------
// The host-pointer work() of the blocks that copy straight from and to the caller's pageable memory (clPowerSpectrum, the
// synthesizer, the resampler, clFEngine, clSignalSource, clCostasLoop, clxcorrelate_fft_vcf): device scratch and the piece loop.
// ---------------------------------------------------------------------------
// Grow-only device scratch of a handle; sizes are bytes.  The caller holds the handle's lock and has set the device, and nothing
// queued may still use the buffer when reserve() has to grow it (these paths wait for their stream after every piece).
struct DevBuf {
    // no-op when the buffer holds `want` bytes already; otherwise the old block is freed and a new one allocated.  After a failed
    // allocation the buffer is empty, no HIP error is left behind and a later reserve() starts from scratch.
    int reserve(size_t want);
    void release();
    void *get() const { return p; }
    size_t bytes() const { return n; }

private:
    void *p = nullptr;
    size_t n = 0;
};

// The one device workspace of a handle whose work_dev calls may come on different streams (clFFT's multi-pass and unfused chirp-z
// routes, clPowerSpectrum, clFEngine's generic route): a DevBuf, an event behind its last user and that user's stream.  The caller
// holds the handle's lock from acquire() to release() and has set the device.
struct DevWorkspace {
    // `st` is the next user and needs `bytes`: if the last user was another stream, st waits for it (on the same stream order is
    // given already); if the buffer has to grow while it has been used, the host waits for that user first, since its kernels may
    // still work on the block that is freed.  A failed allocation leaves the buffer empty (DevBuf::reserve).
    int acquire(size_t bytes, hipStream_t st);
    // after the call's last launch.  Nothing is recorded while st is being captured: a graph orders its own nodes, and an event
    // recorded in a capture is no event for an eager call to wait on.
    int release(hipStream_t st);
    // the host waits for the last user (before something its kernels read is freed); no user yet: nothing to wait for
    int wait();
    void destroy();
    void *get() const { return buf.get(); }
    size_t bytes() const { return buf.bytes(); }
    hipStream_t last_stream() const { return last; }

private:
    DevBuf buf;
    hipEvent_t done = nullptr;  // made by the first acquire
    hipStream_t last = nullptr;
    bool used = false;
};

// units in a piece of a call of `total` >= 1 units that would like `want` per piece
template <class T> static inline T mi355_piece_units(T want, T total) { return want < 1 ? 1 : want > total ? total : want; }

// The piece loop of such a work(): units [0, total) in pieces of `per` (the last one ragged), strictly one after the other on
// ctx->stream[0].  piece(first, count, stream) -> MI355_* queues its copies from the caller's memory, its launches and its copies
// to the caller's memory; the stream is waited for before the next piece starts, so a piece may reuse the scratch of the one
// before.  On the first non-zero code, from piece() or from the wait, the stream is waited for once more (whatever that wait says)
// and the code is returned: no copy from or to the caller's arrays outlives the call, and no later piece is started.
template <class T, class Piece> int mi355_pageable_run(mi355_ctx *ctx, T total, T per, Piece &&piece)
{
    hipStream_t st = ctx->stream[0];
    per = mi355_piece_units(per, total);
    const int rc = [&]() -> int {
        for (T first = 0; first < total; first += per) {
            const int prc = piece(first, total - first < per ? total - first : per, st);
            if (prc) return prc;
            MI355_HIP(hipStreamSynchronize(st));
        }
        return MI355_OK;
    }();
    if (rc != MI355_OK) (void)hipStreamSynchronize(st);
    return rc;
}
