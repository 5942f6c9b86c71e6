"""CPU (no GPU needed): cvxi::DeviceCall (cpuvox_amd/csrc/cvx_context.h), the owner of the device scratch and the event pair of one world call,
compiled for the host through tests/device_call_rules.cpp and run over counting stand-ins for the runtime.  The program is its own executable,
built with -fsanitize=address,undefined (nothing is loaded into Python), and checks that

- every allocated block and every created event is released exactly once: on the success path, on an early failure after one allocation, on a
  failure after Begin and before any allocation, and when a call asks for more blocks than the fixed array holds;
- a kept block is not released and an adopted start event is not destroyed;
- the failure path maps hipErrorOutOfMemory to CVX_ERR_CAPACITY (or the caller's code), clears the thread's last error then and only then, and
  maps everything else to CVX_ERR_HIP."""
import subprocess

import ruleslib


def test_device_call_ownership(tmp_path):
    program = ruleslib.build("device_call_rules", tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", link_library=False)
    run = subprocess.run([program], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failed")
