"""HostPipe's staging-pipeline driver (csrc/common.h HostPipe::run, csrc/hostpipe.hip), which carries the host-pointer work() of
clMathOp, clMathConst, clFilter, clFFT, the channelizer, the translating filter, the beamformer and the dedisperser: its slot
bookkeeping runs on the CPU over synchronous host stubs of the HIP runtime calls it makes, under AddressSanitizer and UBSan
(tests/hostpipe_host_main.cc): a program of its own, nothing loaded into python.  Placement on exact-size buffers over 1 .. 9 chunks
and 1, 2 and 4 slots, the wait before a slot is refilled, zero-byte outputs, the drain after a failed launch or runtime call, and
custom delivery.  The blocks themselves run through it on the GPU (tests/test_device_bounds_gpu.py HOST_CASES and each block's
multi-chunk host test).

The same program then drives mi355_pageable_run, the piece loop of the seven blocks that copy from pageable memory, and DevBuf,
their device scratch: 1 .. 5 pieces with a ragged last one over two inputs (one with a history overlap) and two outputs on
exact-size buffers, the order H2D.. LAUNCH D2H.. STREAM_SYNC per piece, the clamp of the piece size, the wait behind a failed
launch, a failed copy (every one of a call's sixteen) and a failed wait, with nothing logged after it and no output byte of a later
piece touched; and DevBuf's keep / free-then-allocate / failed-allocation / release behaviour against the live-allocation count.

Last comes DevWorkspace, the stream-ordered workspace of clFFT, clPowerSpectrum and clFEngine: no wait at the first acquire or on
the same stream, one stream-wait on the event for another stream, the host's event wait before free and malloc when a used buffer
grows (none for an unused one), a failed allocation that leaves it empty, no event record under capture, and destroy."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "gr-clenabled_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_driver_bookkeeping_under_sanitizers(tmp_path):
    """host code only, a program of its own: no device, nothing loaded into python"""
    exe = tmp_path / "hostpipe_host"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "hostpipe_host_main.cc"), "-x", "c++", os.path.join(CSRC, "hostpipe.hip"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hostpipe host ok" in r.stdout, r.stdout + r.stderr
