"""The base of the C++ block units (host/lib/block_base.h: the two error checks, the context and handle owners, "create or throw", the
log sink installed once) on the CPU over the stub context of tests/host_stub.h, under AddressSanitizer and UBSan
(tests/block_base_host_main.cc): a program of its own, nothing loaded into python."""
import os

import host_layer


def test_base_under_sanitizers(tmp_path):
    host_layer.runs_under_sanitizers(tmp_path, "block_base", [], extra=["-I", os.path.join(host_layer.HOST, "lib")])
