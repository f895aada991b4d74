// HostPipe (common.h): the staging buffers and per-slot events of the host-pointer work() path, DevBuf, the device scratch of
// the pageable host paths, and DevWorkspace, the stream-ordered workspace of a handle.  This unit and the drivers, HostPipe::run and mi355_pageable_run in common.h, use the HIP runtime's host
// API only, so that tests/hostpipe_host_main.cc can compile them with a host compiler over stubs of those calls.
#include "common.h"

int DevBuf::reserve(size_t want)
{
    if (n >= want) return MI355_OK;
    void *old = p;
    p = nullptr;
    n = 0;
    if (old) MI355_HIP(hipFree(old));
    const hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        (void)hipGetLastError();
        mi355_set_error("hipMalloc of %zu bytes of device scratch -> %s", want, hipGetErrorString(e));
        return MI355_ERR_HIP;
    }
    n = want;
    return MI355_OK;
}

void DevBuf::release()
{
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
}

int DevWorkspace::acquire(size_t bytes, hipStream_t st)
{
    if (!done) MI355_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    if (used && last != st) MI355_HIP(hipStreamWaitEvent(st, done, 0));
    if (bytes > buf.bytes() && used) MI355_HIP(hipEventSynchronize(done));  // kernels of an earlier call still use the old one
    return buf.reserve(bytes);
}

int DevWorkspace::release(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return MI355_OK;
    MI355_HIP(hipEventRecord(done, st));
    last = st;
    used = true;
    return MI355_OK;
}

int DevWorkspace::wait()
{
    if (used) MI355_HIP(hipEventSynchronize(done));
    return MI355_OK;
}

void DevWorkspace::destroy()
{
    buf.release();
    if (done) (void)hipEventDestroy(done);
    done = nullptr;
    last = nullptr;
    used = false;
}

int HostPipe::init(mi355_ctx *c)
{
    ctx = c;
    MI355_HIP(hipSetDevice(c->device));
    for (int s = 0; s < kSlots; s++) MI355_HIP(hipEventCreateWithFlags(&done[s], hipEventDisableTiming));
    return MI355_OK;
}

int HostPipe::ensure(int nin, const size_t *in_bytes, size_t out_bytes, int nslots)
{
    MI355_HIP(hipSetDevice(ctx->device));
    if (nslots < 1) nslots = 1;
    if (nslots > kSlots) nslots = kSlots;
    bool grow = nslots > slots_ready || out_bytes > cap_out;
    for (int i = 0; i < nin; i++) grow = grow || in_bytes[i] > cap_in[i];
    if (!grow) return MI355_OK;
    // (re)allocate every slot in use at the larger of the old and new sizes
    size_t want_in[MAXIN] = {cap_in[0], cap_in[1]}, want_out = cap_out > out_bytes ? cap_out : out_bytes;
    for (int i = 0; i < nin; i++) if (in_bytes[i] > want_in[i]) want_in[i] = in_bytes[i];
    const int upto = nslots > slots_ready ? nslots : slots_ready;
    const int rc = [&]() -> int {
        for (int s = 0; s < upto; s++) {
            for (int i = 0; i < MAXIN; i++) {
                if (want_in[i] == 0 || (want_in[i] == cap_in[i] && s < slots_ready)) continue;
                if (h_in[s][i]) MI355_HIP(hipHostFree(h_in[s][i]));
                h_in[s][i] = nullptr;
                if (d_in[s][i]) MI355_HIP(hipFree(d_in[s][i]));
                d_in[s][i] = nullptr;
                MI355_HIP(hipHostMalloc(&h_in[s][i], want_in[i], hipHostMallocDefault));
                MI355_HIP(hipMalloc(&d_in[s][i], want_in[i]));
            }
            if (want_out && !(want_out == cap_out && s < slots_ready)) {
                if (h_out[s]) MI355_HIP(hipHostFree(h_out[s]));
                h_out[s] = nullptr;
                if (d_out[s]) MI355_HIP(hipFree(d_out[s]));
                d_out[s] = nullptr;
                MI355_HIP(hipHostMalloc(&h_out[s], want_out, hipHostMallocDefault));
                MI355_HIP(hipMalloc(&d_out[s], want_out));
            }
        }
        return MI355_OK;
    }();
    if (rc != MI355_OK) {
        // a slot may be half replaced: drop all staging (the old capacities would vouch for buffers that no longer exist) and leave no
        // sticky HIP error behind; the next call allocates from scratch
        (void)hipGetLastError();
        for (int s = 0; s < kSlots; s++) {
            for (int i = 0; i < MAXIN; i++) {
                if (h_in[s][i]) (void)hipHostFree(h_in[s][i]);
                if (d_in[s][i]) (void)hipFree(d_in[s][i]);
                h_in[s][i] = d_in[s][i] = nullptr;
            }
            if (h_out[s]) (void)hipHostFree(h_out[s]);
            if (d_out[s]) (void)hipFree(d_out[s]);
            h_out[s] = d_out[s] = nullptr;
        }
        cap_in[0] = cap_in[1] = cap_out = 0;
        slots_ready = 0;
        (void)hipGetLastError();
        return rc;
    }
    for (int i = 0; i < MAXIN; i++) cap_in[i] = want_in[i];
    cap_out = want_out;
    slots_ready = upto;
    return MI355_OK;
}

void HostPipe::release()
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (int s = 0; s < kSlots; s++) {
        for (int i = 0; i < MAXIN; i++) {
            if (h_in[s][i]) (void)hipHostFree(h_in[s][i]);
            if (d_in[s][i]) (void)hipFree(d_in[s][i]);
            h_in[s][i] = d_in[s][i] = nullptr;
        }
        if (h_out[s]) (void)hipHostFree(h_out[s]);
        if (d_out[s]) (void)hipFree(d_out[s]);
        h_out[s] = d_out[s] = nullptr;
        if (done[s]) (void)hipEventDestroy(done[s]);
        done[s] = nullptr;
    }
    cap_in[0] = cap_in[1] = cap_out = 0;
    slots_ready = 0;
}
