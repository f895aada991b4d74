"""The three recipes of the tests/test_*_host.py files (a plain helper module): a unit of the C++ block layer compiles alone without a
warning, a probe source compiles with -Werror, and a stand-alone program (a main under tests/ plus units) runs under AddressSanitizer
and UBSan -- host code only, a program of its own, no device, nothing loaded into python."""
import os
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "gr-clenabled_amd", "host")
INCLUDE = os.path.join(HOST, "include")
INC = ["-I", INCLUDE, "-I", os.path.join(ROOT, "include")]


def unit(block):
    return os.path.join(HOST, "lib", block + "_impl.cc")


def unit_compiles_alone(block):
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only"] + INC + [unit(block)], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr


def probe_compiles(tmp_path, text):
    src = tmp_path / "probe.cc"
    src.write_text(text)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-fsyntax-only"] + INC + [str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def runs_under_sanitizers(tmp_path, name, blocks, extra=()):
    """tests/<name>_host_main.cc plus the units of `blocks`; "<name> host ok" is the program's last line"""
    exe = tmp_path / (name + "_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + INC +
                       [os.path.join(ROOT, "tests", name + "_host_main.cc")] + [unit(b) for b in blocks] + list(extra) + ["-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and name + " host ok" in r.stdout, r.stdout + r.stderr
