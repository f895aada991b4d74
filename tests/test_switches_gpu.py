"""GPU: the kernels and host paths that only an environment switch reaches, and the loops that cut a call into workspace pieces, against
float64 -- the switches read when a handle is created or at every call (tests/switch_cases.py, INPROC; tests/switches.py is the inventory).
The switches read once per process run in child processes: tests/test_switches_once_gpu.py."""
import pytest

import switch_cases as sc
import test_switches_once_gpu as once

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sc.INPROC))
def test_switch_case(gpu, oracle, monkeypatch, name):
    assert not once.BROKEN, "an earlier child process ended on a signal or at its time limit: " + once.BROKEN
    case = sc.INPROC[name]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    sc.install_log(gpu)
    try:
        r = case.fn(gpu, oracle)
    except Exception as e:
        if sc.device_error(e):  # (the library's MI355_ERR_HIP or a torch error that names the device): nothing further of these two files is started
            once.BROKEN = "%s stopped at a device error: %s" % (name, e)
        raise
    finally:
        gpu.set_log_callback(None)
    once.check(case, r)
