"""GPU: voxel models at any orientation and scale into and out of the device-resident world (cvx_world_place_models[_device],
cvx_world_read_model[_device]).

A call is applied to a context and, independently, to the numpy model's volume (tests/modelsmodel.py), from which the expected world is built on
the host (host.WorldSet.from_voxels): read back, LOD 0 .. levelCount must equal it byte for byte and the levels above must be the old world's.
Everything is integers: no comparison has a tolerance.  The worlds are those of tests/test_gpu_world_dense.py: the 128 x 64 x 128 terrain (one
64-voxel step of the kernels per column) and the 32 x 256 x 32 tall world (four steps).  Every case asserts from the model that its input has the
property it is named for before it calls the device."""
import numpy as np
import pytest

import copymodel
import densemodel
import modelsmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _dense, _world
from test_gpu_world_copy import _assert_levels
from test_gpu_world_dense import TALL, _any_world, _boundaries, _tall_solid
from test_gpu_world_edit import DIMS, _check_world, _context, _frames, _terrain
from test_world_models_cpu import (CARVE, FILL, OPS, PAINT, REPLACE, as_dicts, forward_about_centre, identity_at, mixed_call, model_size, quarter_forward,
                                   random_model, rotation, tilt)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return DIMS, solid, colour, _world(solid, colour)


@pytest.fixture(scope="module")
def world_tall():
    solid = _tall_solid()
    colour = _dense(solid)
    return TALL, solid, colour, _any_world(TALL, solid, colour)


def _open(world):
    ctx = gpu.Context(0)
    ctx.upload_world(world[3])
    return ctx


def _place_and_compare(world, models, instances, level_count, label, render=False):
    """One call on a fresh context and on the model; the read-back world against the world built from the model's volume.  Returns the model's
    (solid, colour)."""
    dims, solid, colour, ws_a = world
    s, c = modelsmodel.place(solid, colour, models, as_dicts(instances))
    assert ((s != solid) | (c != colour)).any(), f"{label} changes nothing"
    ctx = _context(ws_a) if render else _open(world)
    try:
        ms = ctx.place_models(models, instances, level_count)
        assert ms > 0.0
        ws_b = _any_world(dims, s, c)
        try:
            _assert_levels(ctx, ws_b, ws_a, level_count, label)
            if render:  # both render kernels draw the edited world as the oracle draws the expected one
                visited = _check_world(ctx, ws_b, _frames(ws_a)[1:2], label)
                assert visited.sum() > 0
        finally:
            ws_b.close()
    finally:
        ctx.close()
    return s, c


# ---- 1. every op, both worlds, levelCount 0 and 3 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world_name,op_name,level_count", [(w, o, 3) for w in ("terrain", "tall") for o in sorted(OPS)] + [("terrain", "replace", 0), ("tall", "fill", 0)])
def test_every_op_reads_back_as_the_model(world_a, world_tall, world_name, op_name, level_count):
    world = world_a if world_name == "terrain" else world_tall
    dims, solid, colour, _ = world
    op = OPS[op_name]
    names, models, instances = mixed_call(np.random.default_rng(7 + op), dims, op)
    dicts = as_dicts(instances)
    dets = {n: np.linalg.det(np.array(dicts[k]["m"], dtype=np.float64) / 65536) for n, k in names.items()}
    assert dets["negative determinant"] < 0 < dets["yaw 45"], "a mirrored instance"
    assert abs(dets["scale 2"]) < 0.2 and abs(dets["scale 1/2"]) > 7, "magnified and minified instances (toModel is the inverse)"
    outside = dicts[names["partly outside"]]
    assert any(outside["box_min"][i] < 0 or outside["box_max"][i] > dims[i] for i in range(3)) and modelsmodel.rectangle([outside], dims, 0) is not None
    assert model_size(models[2])[1] == 70, "a model taller than a wave"
    if op == CARVE:
        assert all(argb is None and mask is not None for argb, mask in models), "mask-only models"
    else:
        assert any(mask is None for _, mask in models) and any(mask is not None for _, mask in models), "models with argb only and with a mask"
    # columns of the rounded rectangle that no instance's box covers: they are re-encoded, their bytes unchanged
    x0, z0, size_x, size_z = modelsmodel.rectangle(dicts, dims, level_count)
    covered = np.zeros((dims[0], dims[2]), dtype=bool)
    for d in dicts:
        covered[max(d["box_min"][0], 0):d["box_max"][0], max(d["box_min"][2], 0):d["box_max"][2]] = True
    assert not covered[x0:x0 + size_x, z0:z0 + size_z].all(), "every column of the rectangle is under a box"
    _place_and_compare(world, models, instances, level_count, f"{world_name}, {op_name}, levelCount {level_count}")


# ---- 2. runs at and across the steps ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", [REPLACE, FILL])
def test_runs_at_and_across_the_steps(world_tall, op):
    """A model as tall as the world, turned a quarter about y (y stays exact), whose columns hold runs that end exactly at 63 | 64 and
    127 | 128, start there, cross 64 / 128 / 192 and span three steps."""
    dims, solid, colour, _ = world_tall
    spans = [[(10, 64)], [(64, 128)], [(60, 190)], [(0, 64), (65, 128), (129, 192), (193, 256)], [(63, 65), (127, 129), (191, 193)]]
    size = (len(spans), TALL[1], 3)
    mask = np.zeros((size[0], size[2], size[1]), dtype=bool)
    for k, column in enumerate(spans):
        for lo, hi in column:
            mask[k, :, lo:hi] = True
    argb = random_model(np.random.default_rng(4), size, zeros=0.0)[0]
    assert _boundaries(mask[0, 0]) == {10, 64} and _boundaries(mask[1, 0]) == {64, 128} and _boundaries(mask[2, 0]) == {60, 190}
    assert {s // 64 for s in range(60, 190)} == {0, 1, 2}, "a run that spans three steps"
    assert _boundaries(mask[4, 0]) == {63, 65, 127, 129, 191, 193}, "runs that cross the steps"
    forward, dst_size = quarter_forward(1, size, (9, 0, 4))
    inst = gpu.model_instance(forward, size, 0, op)
    s, c = _place_and_compare(world_tall, [(argb, mask)], [inst], 5, f"op {op}")
    placed = [s[9 + x, :, 4 + z] for x in range(dst_size[0]) for z in range(dst_size[2])]
    if op == REPLACE:
        assert any(_boundaries(col) == {60, 190} for col in placed) and any(_boundaries(col) == {64, 128} for col in placed)
    else:
        assert any(col[63] and col[64] for col in placed) and any(col[127] and col[128] for col in placed), "runs across the steps"


# ---- 3. the cull: 1, 64, 65 and 130 instances over a column, in order ------------------------------------------------------------------------------

HEIGHTS = (6, 7, 8, 9, 10)


def _chain_models(rng):
    """Five mask-only columns, one per height, then fifty coloured ones, ten per height."""
    masks = [(None, np.ones((1, 1, h), dtype=bool)) for h in HEIGHTS]
    coloured = [(np.full((1, 1, HEIGHTS[j % 5]), 0xFF000000 | int(rng.integers(1, 1 << 24)), dtype=np.uint32), None) for j in range(50)]
    return masks + coloured


def _chain(column, count):
    """`count` instances over world column `column`: CARVE, FILL, PAINT in turn, models of one column each, shifted in y, so that a voxel's fate
    depends on the order."""
    out = []
    for k in range(count):
        op = (CARVE, FILL, PAINT)[k % 3]
        model = k % 5 if op == CARVE else 5 + k % 5 + 5 * ((k // 5) % 10)
        out.append(identity_at((column[0], 3 + (k * 7) % 23, column[1]), (1, HEIGHTS[k % 5], 1), model, op))
    return out


def test_the_cull_keeps_every_instance_in_order(world_a):
    dims, solid, colour, _ = world_a
    columns = {1: (20, 20), 64: (40, 21), 65: (60, 22), 130: (80, 23)}
    pool = _chain_models(np.random.default_rng(12))
    instances = [inst for count, column in columns.items() for inst in _chain(column, count)]
    # interleave the chains so that the list's order, not the column's, is what the cull has to keep
    instances = [instances[k] for k in np.argsort([k % 7 for k in range(len(instances))], kind="stable")]
    dicts = as_dicts(instances)
    for count, (x, z) in columns.items():
        covering = [d for d in dicts if d["box_min"][0] <= x < d["box_max"][0] and d["box_min"][2] <= z < d["box_max"][2]]
        assert len(covering) == count
        assert all(model_size(pool[d["model"]])[1] == d["box_max"][1] - d["box_min"][1] for d in covering)
    assert len(instances) == 260
    s, c = modelsmodel.place(solid, colour, pool, dicts)
    r, rc = modelsmodel.place(solid, colour, pool, dicts[::-1])
    for count, (x, z) in columns.items():
        if count > 1:
            assert (s[x, :, z] != r[x, :, z]).any() or (c[x, :, z] != rc[x, :, z]).any(), f"{count} instances: the result does not depend on their order"
    _place_and_compare(world_a, pool, instances, 3, "the chains")


def test_4096_instances_of_one_voxel(world_a):
    dims, solid, colour, _ = world_a
    model = (np.full((1, 1, 1), 0xFFC0FFEE, dtype=np.uint32), None)
    instances = [identity_at((32 + k // 64, 40 + (k * 5) % 17, 32 + k % 64), (1, 1, 1), 0, FILL) for k in range(gpu.MODELS_MAX_INSTANCES)]
    s, c = modelsmodel.place(solid, colour, [model], as_dicts(instances))
    assert len(instances) == 4096 and int((c == 0xFFC0FFEE).sum()) == 4096 and int((s & ~solid).sum()) > 3000
    _place_and_compare(world_a, [model], instances, 3, "4096 instances")


# ---- 4. rendering -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world_name", ["terrain", "tall"])
def test_the_edited_world_renders_as_the_rebuild(world_a, world_tall, world_name):
    world = world_a if world_name == "terrain" else world_tall
    names, models, instances = mixed_call(np.random.default_rng(31), world[0], REPLACE)
    for k, inst in enumerate(instances):  # every op in one call
        inst.op = (REPLACE, FILL, PAINT, FILL)[k % 4]
    assert {i.op for i in instances} == {REPLACE, FILL, PAINT}
    _place_and_compare(world, models, instances, 5, f"{world_name}, rendered", render=True)


# ---- 5. torch tensors, the read, the round trip ---------------------------------------------------------------------------------------------------

def _i32(words):
    return words.view(np.int32)


def test_device_variants_take_torch_tensors(world_a):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    dims, solid, colour, ws_a = world_a
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(8)
    size = (12, 14, 10)
    argb, mask = random_model(rng, size, with_mask=True)
    inst = [gpu.model_instance(forward_about_centre(1.5 * tilt(), size, (60, 14, 70)), size, 0, REPLACE),
            gpu.model_instance(forward_about_centre(rotation(1, 45), size, (30, 10, 30)), size, 1, CARVE)]
    models = [(argb, None), (None, mask)]
    s, c = modelsmodel.place(solid, colour, models, as_dicts(inst))
    assert ((s != solid) | (c != colour)).any()
    ctx = _open(world_a)
    try:
        t_argb = torch.from_numpy(_i32(argb)).to(dev).contiguous()
        t_mask = torch.from_numpy(mask.view(np.uint8)).to(dev).contiguous()
        torch.cuda.synchronize()
        ms = ctx.place_models_device([(size, t_argb.data_ptr(), 0), (size, 0, t_mask.data_ptr())], inst, 5)
        assert ms > 0.0
        ws_b = _any_world(dims, s, c)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, "tensors placed")
        finally:
            ws_b.close()
        # a tilted sample of the edited world into tensors on a stream of torch's (the place has finished: the call returns when the edit is done)
        forward = forward_about_centre(tilt(), (20, 24, 16), (60, 14, 70))
        to_world = gpu.model_instance(np.linalg.inv(np.vstack([forward, [0, 0, 0, 1]]))[:3], dims).toModel
        d = modelsmodel.from_struct(gpu.model_instance(np.linalg.inv(np.vstack([forward, [0, 0, 0, 1]]))[:3], dims))
        want_argb, want_mask = modelsmodel.read(s, c, (20, 24, 16), d["m"], d["t"])
        assert want_mask.any() and not want_mask.all()
        out_argb = torch.full((20, 16, 24), -1, dtype=torch.int32, device=dev)
        out_mask = torch.full((20, 16, 24), 7, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ctx.read_model_device((20, 24, 16), to_world, out_argb.data_ptr(), out_mask.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert (out_argb.cpu().numpy().view(np.uint32) == want_argb).all() and (out_mask.cpu().numpy().astype(bool) == want_mask).all()
        # the host variant reads the same, either array alone too
        got_argb, got_mask = ctx.read_model((20, 24, 16), to_world)
        assert (got_argb == want_argb).all() and (got_mask == want_mask).all()
        only_argb, none = ctx.read_model((20, 24, 16), to_world, want_solid=False)
        assert none is None and (only_argb == want_argb).all()
    finally:
        ctx.close()


def test_read_with_the_identity_is_the_dense_read(world_a):
    dims, solid, colour, _ = world_a
    at, size = (-3, 5, 100), (40, 70, 31)
    ctx = _open(world_a)
    try:
        to_world = identity_at([-a for a in at], size).toModel  # toModel of a model at -at: world = model + at
        got_argb, got_mask = ctx.read_model(size, to_world)
        want_argb, want_mask = densemodel.read(solid, colour, (at, tuple(at[i] + size[i] for i in range(3))))
        dense_argb, dense_mask = ctx.read_voxels(at, tuple(at[i] + size[i] for i in range(3)))
        assert want_mask.any() and not want_mask.all()
        assert (got_argb == want_argb).all() and (got_mask == want_mask).all() and (got_argb == dense_argb).all() and (got_mask == dense_mask).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("transform", [1, 6, 11])
def test_read_and_place_at_a_quarter_turn_is_the_copy(world_a, transform):
    """read_model_device of a box through a quarter-turn map, placed back as it lies with CVX_COPY_REPLACE: the round trip is exact and equals
    cvx_world_copy of that box under the same transform."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    dims, solid, colour, ws_a = world_a
    dev = torch.device("cuda", 0)
    src_min, src_max, dst = (20, 4, 30), (33, 24, 39), (70, 10, 60)
    size = tuple(src_max[i] - src_min[i] for i in range(3))
    forward, dst_size = quarter_forward(transform, size, (0, 0, 0))
    # the map model voxel -> world voxel is the inverse of w -> forward(w - srcMin): the helper's toModel of that matrix
    matrix = np.concatenate([forward[:, :3], (forward[:, 3] - forward[:, :3] @ np.array(src_min, dtype=np.float64))[:, None]], axis=1)
    to_world = gpu.model_instance(matrix, dims).toModel
    d = modelsmodel.from_struct(gpu.model_instance(matrix, dims))
    want_argb, want_mask = modelsmodel.read(solid, colour, dst_size, d["m"], d["t"])
    box = copymodel.transformed_box(solid[src_min[0]:src_max[0], src_min[1]:src_max[1], src_min[2]:src_max[2]], transform)
    assert (want_mask.transpose(0, 2, 1) == box).all() and box.any() and not box.all(), "the read is the turned box"
    placement = dict(srcMin=src_min, srcMax=src_max, dst=dst, transform=transform, op=REPLACE, move=0)
    s, c = copymodel.apply_copies(solid, colour, [placement])
    ctx, ref = _open(world_a), _open(world_a)
    try:
        n = dst_size[0] * dst_size[1] * dst_size[2]
        t_argb = torch.zeros(n, dtype=torch.int32, device=dev)
        t_mask = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ctx.read_model_device(dst_size, to_world, t_argb.data_ptr(), t_mask.data_ptr())
        assert ctx.place_models_device([(dst_size, t_argb.data_ptr(), t_mask.data_ptr())], [identity_at(dst, dst_size)], 5) > 0.0
        assert ref.copy([placement], 5) > 0.0
        for level in range(6):
            assert ctx.read_level(level) == ref.read_level(level), f"LOD {level}"
        ws_b = _any_world(dims, s, c)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, f"transform {transform}")
        finally:
            ws_b.close()
    finally:
        ctx.close()
        ref.close()


# ---- 6. errors and calls that do nothing ----------------------------------------------------------------------------------------------------------

def test_a_failing_call_leaves_the_world_alone(world_a):
    dims, solid, colour, _ = world_a
    model = random_model(np.random.default_rng(1), (5, 6, 7))
    instances = [gpu.model_instance(forward_about_centre(rotation(1, 20 * k), (5, 6, 7), (20 + 15 * k, 12, 40)), (5, 6, 7), 0, REPLACE) for k in range(5)]
    assert ((modelsmodel.place(solid, colour, [model], as_dicts(instances))[0]) != solid).any(), "the call would change the world"
    ctx = _open(world_a)
    try:
        before = [ctx.read_level(k) for k in range(6)]
        stats = ctx.edit_stats()
        for field, value, message in (("op", 7, "instance 3: bad op"), ("model", 1, "instance 3: model"), ("boxMax", None, "instance 3: the box")):
            bad = [gpu.ModelInstance.from_buffer_copy(bytes(i)) for i in instances]
            if value is None:
                bad[3].boxMax[1] = bad[3].boxMin[1]
            else:
                setattr(bad[3], field, value)
            with pytest.raises(gpu.CvxError, match=message):
                ctx.place_models([model], bad, 5)
        with pytest.raises(gpu.CvxError, match="levelCount"):
            ctx.place_models([model], instances, 6)
        assert [ctx.read_level(k) for k in range(6)] == before and ctx.edit_stats() == stats
        assert ctx.place_models([model], instances, 5) > 0.0
        assert ctx.read_level(0) != before[0]
    finally:
        ctx.close()
    fresh = gpu.Context(0)
    try:  # before an upload
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.place_models([model], instances)
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.read_model((2, 2, 2), instances[0].toModel)
    finally:
        fresh.close()


def test_boxes_outside_the_world_do_nothing(world_a):
    dims, solid, colour, ws_a = world_a
    model = random_model(np.random.default_rng(2), (4, 4, 4))
    instances = [identity_at((dims[0] + 1, 0, 0), (4, 4, 4)), identity_at((3, dims[1], 3), (4, 4, 4), 0, FILL), identity_at((3, 3, -4), (4, 4, 4), 0, CARVE)]
    assert modelsmodel.rectangle(as_dicts(instances), dims, 0) is None
    ctx = _open(world_a)
    try:
        ctx.read_level(0)  # (lays the arena out: the statistics from here on are the arena's)
        stats = ctx.edit_stats()
        assert ctx.place_models([model], instances, 5) == 0.0
        _assert_levels(ctx, ws_a, ws_a, 5, "outside")
        assert ctx.edit_stats() == stats and stats[0] > 0 and stats[1:] == (0, 0)
    finally:
        ctx.close()
