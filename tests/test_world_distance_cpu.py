"""CPU (no GPU needed): the rules behind cvx_world_distance (cpuvox_amd/csrc/cvx_distance.h), compiled for the host through
tests/distance_rules.cpp, against the independent dense model of tests/distancemodel.py, element for element.

- The model against itself: the padded min-plus, the sparse brute force and a plain triple loop agree on small boxes.
- Random dense and sparse worlds of (32, 32, 32) and (16, 256, 16) uploaded into a host-only context: cvxb::DistanceField -- the three passes
  an element at a time, through the functions the kernels call -- over boxes that stick out of the world, for the three modes, R = 1, 2, 3,
  7, 20 and solidOutside 0, 0x04, 0x3F and +X alone.
- Named single-column cases: an empty column, a full one, runs touching y = 0 and dimY - 1, boxes wholly below, above and beside the world.
- The calls without a context / world, the Python wrapper's own checks, the README's export count."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import distancemodel
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = gpu.DISTANCE_FAR
MODES = {"to solid": gpu.DISTANCE_TO_SOLID, "to air": gpu.DISTANCE_TO_AIR, "signed": gpu.DISTANCE_SIGNED}
OUTSIDES = (0, 0x04, 0x3F, 0x02)  # nothing, the ground (the default), every side, +X alone


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("distance_rules", tmp_path_factory.mktemp("distance"))


def test_constants_are_the_headers():
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu.h")).read()
    assert re.search(r"#define CVX_DISTANCE_FAR 0x7FFFFFFF\b", header) and FAR == 0x7FFFFFFF == distancemodel.FAR
    assert re.search(r"CVX_DISTANCE_TO_SOLID = 0, CVX_DISTANCE_TO_AIR = 1, CVX_DISTANCE_SIGNED = 2", header)
    assert (gpu.DISTANCE_TO_SOLID, gpu.DISTANCE_TO_AIR, gpu.DISTANCE_SIGNED) == (0, 1, 2) == (distancemodel.TO_SOLID, distancemodel.TO_AIR, distancemodel.SIGNED)


# ---- the model against itself ---------------------------------------------------------------------------------------------------------------------

def test_the_three_models_agree_on_small_boxes():
    rng = np.random.default_rng(5)
    solid = rng.random((6, 5, 7)) < 0.15
    solid[2, 1:4, 3] = True
    checked = 0
    for box in (((0, 0, 0), (6, 5, 7)), ((-3, -2, 4), (2, 3, 9)), ((5, 4, -4), (9, 8, 1))):
        for R, outside in ((1, 0), (2, 0x04), (3, 0x3F), (3, 0x10), (2, 0x09)):
            for mode in MODES.values():
                want = distancemodel.brute_field(solid, box, R, mode, outside)
                got = distancemodel.field(solid, box, R, mode, outside)
                assert (got == want).all(), (box, R, outside, mode)
                checked += 1
            if outside == 0:
                points = np.argwhere(solid)
                assert (distancemodel.sparse_field(points, box, R) == distancemodel.brute_field(solid, box, R, gpu.DISTANCE_TO_SOLID, 0)).all()
    assert checked == 45
    # R larger than the box and the world: the windows reach over both
    box = ((1, 1, 1), (4, 3, 4))
    assert (distancemodel.field(solid, box, 9, gpu.DISTANCE_SIGNED, 0x04) == distancemodel.brute_field(solid, box, 9, gpu.DISTANCE_SIGNED, 0x04)).all()


def test_the_model_agrees_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    solid = _pick_world(np.random.default_rng(1), (32, 32, 32), False)[0]
    for R in (1, 3, 8):
        # scipy sees only the array: compare where the nearest solid voxel cannot lie outside it (the ball of radius R stays inside)
        edt = np.rint(ndimage.distance_transform_edt(~solid) ** 2).astype(np.int64)
        want = np.where(edt <= R * R, edt, FAR)[R:-R, R:-R, R:-R].transpose(0, 2, 1)
        got = distancemodel.field(solid, ((R, R, R), (32 - R, 32 - R, 32 - R)), R, gpu.DISTANCE_TO_SOLID, 0)
        assert (got == want).all(), R


# ---- the rule header -----------------------------------------------------------------------------------------------------------------------------

def _run_fields(rules, tmp_path, ws, queries):
    """queries: (box_min, box_max, R, mode, solid_outside) -> the fields of cvxb::DistanceField, each of shape (X, Z, Y)."""
    info = ws.info(0)
    blob, src, dst = tmp_path / "world.bin", tmp_path / "queries.bin", tmp_path / "fields.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    words = [[*lo, *[hi[a] - lo[a] for a in range(3)], R, mode, outside] for lo, hi, R, mode, outside in queries]
    src.write_bytes(np.array(words, dtype=np.int32).tobytes())
    subprocess.check_call([rules, "fields", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(src), str(dst)])
    raw = np.frombuffer(dst.read_bytes(), dtype=np.int32)
    fields, at = [], 0
    for lo, hi, *_ in queries:
        shape = (hi[0] - lo[0], hi[2] - lo[2], hi[1] - lo[1])
        n = shape[0] * shape[1] * shape[2]
        fields.append(raw[at:at + n].reshape(shape))
        at += n
    assert at == raw.size
    return fields


def _random_world(rng, dims, sparse):
    if not sparse:
        return _pick_world(rng, dims, False)
    solid = rng.random(dims) < 0.002
    x, y, z = np.nonzero(solid)
    ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF336699, dtype=np.uint32), threads=2)
    return solid, None, ws


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((32, 32, 32), True, 2), ((16, 256, 16), False, 3), ((16, 256, 16), True, 4)])
def test_rule_header_matches_the_model(rules, tmp_path, dims, sparse, seed):
    rng = np.random.default_rng(seed)
    solid, _, ws = _random_world(rng, dims, sparse)
    assert solid.any() and not solid.all() and (not sparse or solid.mean() < 0.01)
    dx, dy, dz = dims
    # the world with a rim of 2 around it for the small radii; for R = 7 and 20 a box across the world's (+X, +Y, -Z) corner
    whole = ((-2, -2, -2), (dx + 2, dy + 2, dz + 2))
    corner = ((dx - 9, dy - 20, -4), (dx + 3, dy + 6, 7))
    queries = [(whole if R <= 3 else corner) + (R, mode, outside) for R in (1, 2, 3, 7, 20) for mode in MODES.values() for outside in OUTSIDES]
    try:
        fields = _run_fields(rules, tmp_path, ws, queries)
    finally:
        ws.close()
    near = far = negative = 0
    for (lo, hi, R, mode, outside), got in zip(queries, fields):
        want = distancemodel.field(solid, (lo, hi), R, mode, outside)
        bad = got != want
        assert not bad.any(), f"R {R} mode {mode} solidOutside {outside:#x} box {lo} .. {hi}: {int(bad.sum())} of {bad.size} differ, first at " \
                              f"{np.argwhere(bad)[0].tolist()} (x, z, y): {got[bad][0]} for {want[bad][0]}"
        near += int(((want > 0) & (want != FAR)).sum())
        far += int((want == FAR).sum())
        negative += int((want < 0).sum())
    assert near > 1000 and far > 1000 and negative > 1000, (near, far, negative)


def _column_world():
    """(16, 32, 16): column (2, 2) full, (12, 4) with runs touching y = 0 and y = 31, (8, 8) and everything within 5 of it empty, (13, 13) one
    voxel; a floor one voxel thick under the x < 3 part."""
    dims = (16, 32, 16)
    solid = np.zeros(dims, dtype=bool)
    solid[:3, 0, :] = True
    solid[2, :, 2] = True
    solid[12, 0:5, 4] = True
    solid[12, 27:32, 4] = True
    solid[13, 15, 13] = True
    x, y, z = np.nonzero(solid)
    return dims, solid, host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF808080, dtype=np.uint32), threads=2)


def test_named_column_cases(rules, tmp_path):
    dims, solid, ws = _column_world()
    assert solid[2, :, 2].all(), "a full column"
    assert not solid[3:14, :, 5:12].any(), "an empty column with empty neighbours"
    assert solid[12, 0, 4] and solid[12, 31, 4] and not solid[12, 5:27, 4].any(), "runs touching y = 0 and dimY - 1"
    boxes = {
        "empty column": ((8, -3, 8), (9, 35, 9)),
        "full column": ((2, -3, 2), (3, 35, 3)),
        "runs at both ends": ((12, -3, 4), (13, 35, 5)),
        "around the full column": ((0, 10, 0), (5, 14, 5)),
        "wholly below": ((1, -12, 1), (6, -4, 5)),
        "wholly above": ((10, 36, 2), (14, 41, 6)),
        "beside -x": ((-9, 2, 1), (-3, 8, 5)),
        "beside +z": ((10, 0, 19), (14, 32, 24)),
        "beside the corner": ((17, 33, 17), (20, 36, 20)),
    }
    for name, (lo, hi) in boxes.items():
        outside = any(hi[a] <= 0 or lo[a] >= dims[a] for a in range(3))
        assert outside == (name.startswith("wholly") or name.startswith("beside")), name
    queries = [box + (R, mode, out) for box in boxes.values() for R in (1, 3, 7) for mode in MODES.values() for out in OUTSIDES]
    try:
        fields = _run_fields(rules, tmp_path, ws, queries)
    finally:
        ws.close()
    for (lo, hi, R, mode, outside), got in zip(queries, fields):
        want = distancemodel.field(solid, (lo, hi), R, mode, outside)
        assert (got == want).all(), (lo, hi, R, mode, outside, got.ravel().tolist(), want.ravel().tolist())
    # what the names promise, from the model: the full column has no air of its own, the empty one no solid
    full = distancemodel.field(solid, boxes["full column"], 7, gpu.DISTANCE_TO_AIR, 0x0C)[0, 0]
    assert (full[3:35] == 1).all() and full[0] == 10, "with solid below and above, the nearest air of a full column is beside it; (2, -3, 2)'s is (3, 0, 2)"
    empty = distancemodel.field(solid, boxes["empty column"], 3, gpu.DISTANCE_TO_SOLID, 0)
    assert (empty == FAR).all()
    below = distancemodel.field(solid, boxes["wholly below"], 7, gpu.DISTANCE_SIGNED, 0x04)
    assert (below < 0).all() and below[0, 2, 7] == -29 and below[3, 2, 7] == -25 and below[3, 2, 0] == -FAR, \
        "the ground is solid; above (4, -5, 3) air starts at y = 0, above (1, -5, 3) lies the floor: its nearest air is (3, 0, 3)"


# ---- entry points -------------------------------------------------------------------------------------------------------------------------------

def test_calls_fail_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)
    out = (C.c_int32 * 8)()
    assert L.cvx_world_distance(None, lo, hi, 4, 0, 4, out, None) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    assert L.cvx_world_distance_device(None, lo, hi, 4, 0, 4, out, None) == -1
    # a context without a device or world (tests/distance_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 18 + [-3] * 3, codes
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu.h")).read()
    for name in ("cvx_world_distance", "cvx_world_distance_device"):
        assert name in gpu.EXPORTS and re.search(r"\bint " + name + r"\(", header)
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_distance(h, lo, hi, 4, 0, 4, out, None) == -3
        finally:
            L.cvx_destroy(h)


def test_python_wrappers_check_their_boxes():
    ctx = object.__new__(gpu.Context)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.distance(ctx, (0, 0), (1, 1, 1), 4)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.distance_device(ctx, (0, 0, 0), (1, 1, 1, 1), 4, 0)


def test_readme_counts_the_exports():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert len(gpu.EXPORTS) == 83 and f"all {len(gpu.EXPORTS)} exports" in readme and "all 64 exports" in readme
    assert "cvx_world_distance" in readme
