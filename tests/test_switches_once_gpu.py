"""GPU: the switches that are read once per process (a `static` initialiser in csrc/), each group of them in a fresh child process that
starts with the variables set (tests/switch_cases.py, CHILD and GROUPS).  A child is started, never exec'd over this process, one at a
time, under its own time limit; it prints one JSON line per case and the parent asserts on those lines.  If a child ends on a signal or at
its time limit nothing further is started: every later case of this file and of tests/test_switches_gpu.py fails at once."""
import json
import os
import subprocess
import sys

import pytest

import switch_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu
BROKEN = ""    # why no further child may be started
_RESULTS = {}  # group -> {case name: result} or an error text


def check(case, r):
    """the assertions on one case's result (shared with tests/test_switches_gpu.py)"""
    for label, err, bound in r["checks"]:
        print("%-28s %-70s %.3g (bound %.3g)" % (case.name, label, err, bound))
    if case.taken is not None:
        assert r["taken"] is case.taken, "evidence that the switch was acted on: expected %s, the library said %r" % (case.taken, r["evidence"])
    assert r["checks"], "the case compared nothing"
    for label, err, bound in r["checks"]:
        assert err <= bound, (label, err, bound)


def _run_group(group):
    global BROKEN
    if group in _RESULTS:
        return _RESULTS[group]
    assert not BROKEN, "an earlier child process ended on a signal or at its time limit: " + BROKEN
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355_")}
    env.update(sc.GROUPS[group])
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_cases.py"), group], capture_output=True, text=True, timeout=180, env=env)
    except subprocess.TimeoutExpired as e:
        BROKEN = "group %s ran into its time limit; it printed: %s" % (group, (e.stdout or b"")[-2000:])
        _RESULTS[group] = BROKEN
        return BROKEN
    if p.returncode < 0 or p.returncode == sc.FAULT_EXIT or (p.returncode != 0 and sc.DEVICE_ERROR.search(p.stderr[-6000:])):
        BROKEN = "group %s ended on %s; it printed: %s" % (group, "a device error" if p.returncode > 0 else "signal %d" % -p.returncode,
                                                          p.stdout[-2000:] + p.stderr[-2000:])
        _RESULTS[group] = BROKEN
        return BROKEN
    out = {}
    for line in p.stdout.splitlines():
        if line.startswith("CASE "):
            r = json.loads(line[5:])
            out[r["case"]] = r
    if p.returncode != 0 or "GROUP DONE " + group not in p.stdout:
        out["__error__"] = "exit status %d: %s" % (p.returncode, p.stderr[-3000:])
    _RESULTS[group] = out
    return out


@pytest.mark.parametrize("name", list(sc.CHILD))
def test_switch_case_in_a_fresh_process(gpu, name):
    case = sc.CHILD[name]
    res = _run_group(case.group)
    assert isinstance(res, dict), res
    assert name in res, res.get("__error__", "the child printed no line for this case")
    check(case, res[name])
