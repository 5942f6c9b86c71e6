"""CPU (no GPU needed): cvxi::ModelStaging (cpuvox_amd/csrc/cvx_model_call.h), the one device block that holds the host model arrays of the calls
on placed models, compiled for the host through tests/model_staging_rules.cpp and run over counting stand-ins for the runtime.  The program is
its own executable, built with -fsanitize=address,undefined (nothing is loaded into Python), and checks, for three models (argb only, 1 voxel;
solid only, 17 voxels; both, 3 x 5 x 7), the same three on the device, a single 1-voxel solid-only model and an allocation that fails, that

- every array lies at a multiple of 16, argb before solid per model, in model order, no two regions overlap and the total is the sum of the
  rounded sizes;
- the descriptors to upload point into the block exactly where the caller's were not NULL and keep their sizes; with the arrays on the device
  nothing is allocated and the descriptors are the caller's;
- a failed allocation is returned, and cvxi::DeviceCall::Fail then reports the block's bytes;
- every block is released exactly once, by the DeviceCall it was allocated from."""
import subprocess

import ruleslib


def test_model_staging_plan_and_ownership(tmp_path):
    program = ruleslib.build("model_staging_rules", tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", link_library=False)
    run = subprocess.run([program], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("0 failed")
