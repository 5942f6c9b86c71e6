"""-m gpu: the texture row of a side pixel from the batch kernel's approximate end quotients, on the device (cvx_selftest_math op 17, experiment build).

Per sample {y, boundsX, boundsY, bottom.z, top.z, uA, swap} the op computes the reference's row (IEEE quotients, the swap, tex_row_exact), the shipped path's row
and its `certain` flag (tex_ends_approx, tex_run<true>, tex_row_cheap<true>: the very functions the kernel calls, with the hardware's own reciprocals), and the
fall-back's row (tex_row_fallback).  No certain row may differ from the reference's, every fall-back row must equal it, and renderer-shaped samples must be
certain almost always.  The sample families are those of the CPU model of the argument, tests/test_texture_row_inputs_model.py."""
import os

import numpy as np
import pytest

import test_texture_row_inputs_model as M
from cpuvox_amd import gpu

pytestmark = pytest.mark.gpu

GROUPS = 1 << 22


@pytest.fixture
def diag_context():
    """A context of the experiment build (the only one that exports cvx_selftest_math): same sources, same compiler flags, same device functions as the product
    build; `make all` builds it next to the product library, so a missing file is a broken build."""
    path = os.path.join(os.path.dirname(gpu.lib_path()), "libcpuvox_gpu_exp.so")
    assert os.path.exists(path), "libcpuvox_gpu_exp.so not built: run `make -C cpuvox_amd/csrc all` (or __graft_entry__.build())"
    gpu.use_library(path)
    ctx = gpu.Context(0)
    try:
        yield ctx
    finally:
        ctx.close()
        gpu.use_library(None)


def _run(ctx, family, seed, near_integer=True):
    y, bx, by, zb, zt, ua = M.samples(family, seed, GROUPS, near_integer)
    swap = (np.random.default_rng(seed + 1000).random(GROUPS) < 0.5).astype(np.float32)
    a = np.stack([y, bx, by, zb], axis=1).reshape(-1)
    b = np.stack([zt, ua, swap, np.zeros(GROUPS, dtype=np.float32)], axis=1).reshape(-1)
    out = ctx.selftest_math(17, a, b).view(np.int32).reshape(-1, 4)
    reference, shipped, certain, fallback = out[:, 0], out[:, 1], out[:, 2] == 1, out[:, 3]
    cols = (y, bx, by, zb, zt, ua, swap)
    wrong = certain & (shipped != reference)
    assert not wrong.any(), (f"{family}: {wrong.sum()} certain rows differ, e.g. inputs {[c[np.flatnonzero(wrong)[0]] for c in cols]} "
                             f"reference {reference[wrong][0]} shipped {shipped[wrong][0]}")
    bad = fallback != reference
    assert not bad.any(), (f"{family}: {bad.sum()} fall-back rows differ, e.g. inputs {[c[np.flatnonzero(bad)[0]] for c in cols]} "
                           f"reference {reference[bad][0]} fall-back {fallback[bad][0]}")
    return certain.mean()


@pytest.mark.parametrize("family,seed", [("renderer", 101), ("level", 102), ("deep", 103), ("extreme", 104), ("extreme", 105), ("soup", 106), ("soup", 107)])
def test_certain_rows_and_fallback_rows_equal_the_reference_rows(diag_context, family, seed):
    share = _run(diag_context, family, seed)
    print(f"{family} (seed {seed}): certain {share:.4f}")


@pytest.mark.parametrize("family,seed", [("renderer", 111), ("deep", 113), ("level", 112)])
def test_renderer_shaped_rows_stay_certain(diag_context, family, seed):
    """Run lengths as they come; the bar of the narrow form's device test (tests/test_gpu_parity.py).  The level camera is printed, as in the CPU model."""
    share = _run(diag_context, family, seed, near_integer=False)
    print(f"{family} (seed {seed}): certain {share:.4f}")
    if family != "level":
        assert share > 0.97, f"only {share:.4f} of the {family} rows are certain"
