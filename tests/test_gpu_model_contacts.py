"""GPU: where placed voxel models touch each other (cvxp_model_contacts[_device], include/cpuvox_gpu_pair_contacts.h).

A call is made on a context and, independently, on the numpy model (tests/paircontactsmodel.py): results, points and summary must be equal byte
for byte.  Everything is integers: no comparison has a tolerance.  The scenes are those tests/test_model_contacts_cpu.py builds (and runs through
the host build of the rules), plus the ones only the launch can get wrong: more jobs than waves, the capacity, the device tensors.  Every case
asserts from the model that its input has the property it is named for before it calls the device.  All but two tests run on a context with
nothing uploaded: the calls need no world."""
import numpy as np
import pytest
import torch

import contactsmodel
from cpuvox_amd import gpu
from test_gpu_world_contacts import _device_models
from test_gpu_world_dense import _any_world
from test_model_contacts_cpu import (FILL, assert_clipped, assert_cubes, assert_empty, assert_mixed, assert_steps, model_of, same, scene_clipped, scene_cubes,
                                     scene_empty, scene_lattice, scene_mixed, scene_steps)
from test_world_contacts_cpu import CUBE, cube_model, flat_world
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, random_model, rotation

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RESULT_BYTES, POINT_BYTES = 144, 32


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


def _device_call(ctx, models, instances, pairs, capacity, spare=0):
    """One device call into sentinel-filled tensors -> (results, the points tensor's entries as an array, totals)."""
    descriptors, keep = _device_models(models)  # noqa: F841  (keep: the tensors the descriptors point to)
    results = torch.full((len(pairs) * RESULT_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
    points = torch.full(((capacity + spare) * POINT_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda") if capacity + spare else None
    torch.cuda.synchronize()
    handed = points if points is None or not spare else (points[:capacity * POINT_BYTES] if capacity else None)  # (the wrapper takes the tensor's size for the capacity)
    totals, ms = ctx.model_contacts_device(descriptors, instances, pairs, results, handed)
    assert ms > 0.0
    listed = points.cpu().numpy().view(gpu.PAIR_POINT_DTYPE) if points is not None else np.zeros(0, dtype=gpu.PAIR_POINT_DTYPE)
    return results.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE), listed, totals


def _check(ctx, scene, what, device=True):
    """The host call, and the device call, against the model; returns the model's answer."""
    models, instances, pairs = scene
    want = model_of(models, instances, pairs)
    results, points, totals, ms = ctx.model_contacts(models, instances, pairs)
    assert ms > 0.0
    same((results, points, totals), want, what)
    if device:
        same(_device_call(ctx, models, instances, pairs, want[2]["points"]), want, what + " (device)")
    return want


# ---- 1. two cubes, by hand ----------------------------------------------------------------------------------------------------------------------

def test_two_cubes_by_hand(ctx):
    want = _check(ctx, scene_cubes(), "cubes")
    assert_cubes(*want)
    results, points, totals, _ = ctx.model_contacts(*scene_cubes())
    assert_cubes(results, points, totals)
    assert gpu.pair_response(results[0], 0)[2] == 1.0


# ---- 2. the mixed call, box_pairs choosing the pairs -------------------------------------------------------------------------------------------

def test_the_mixed_call(ctx):
    scene = scene_mixed()
    models, instances, pairs = scene
    assert gpu.box_pairs(instances).tolist() == pairs[:-2].tolist(), "the pairs are box_pairs' (and two more)"
    assert_mixed(scene, _check(ctx, scene, "mixed"))
    # pairs=None: the wrapper asks box_pairs itself
    results, points, totals, _ = ctx.model_contacts(models, instances)
    same((results, points, totals), model_of(models, instances, pairs[:-2]), "pairs=None")


# ---- 3. the steps of the walk ------------------------------------------------------------------------------------------------------------------

def test_the_steps_of_the_walk(ctx):
    scene = scene_steps()
    assert_steps(scene, _check(ctx, scene, "steps"))


# ---- 4. bodies clipped by their own boxes ----------------------------------------------------------------------------------------------------------

def test_bodies_clipped_by_their_own_boxes(ctx):
    scene = scene_clipped()
    assert_clipped(scene, _check(ctx, scene, "clipped"))


# ---- 5. pairs with empty intersections -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("only", [False, True])
def test_pairs_with_empty_intersections(ctx, only):
    scene = scene_empty(only)
    want = _check(ctx, scene, "empty")
    assert_empty(scene, want, only)
    if not only:
        return
    # a list asked for when there are no jobs: no walk and no scan is launched, and nothing is written
    models, instances, pairs = scene
    assert want[2]["jobs"] == 0 and want[2]["points"] == 0 and len(want[1]) == 0
    results, points, totals, _ = ctx.model_contacts(models, instances, pairs, capacity=4)
    assert len(points) == 0 and results.tobytes() == want[0].tobytes() and totals == want[2], "a host list of no jobs"
    descriptors, keep = _device_models(models)  # noqa: F841  (keep: the tensors the descriptors point to)
    device_results = torch.full((len(pairs) * RESULT_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
    device_points = torch.full((4 * POINT_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    totals, ms = ctx.model_contacts_device(descriptors, instances, pairs, device_results, device_points)
    assert ms >= 0.0 and totals == want[2] and device_results.cpu().numpy().tobytes() == want[0].tobytes(), "a device list of no jobs"
    assert (device_points.cpu().numpy() == SENTINEL).all(), "no byte of the list is written"


# ---- 6. more pairs than the finish kernel has threads --------------------------------------------------------------------------------------------

def test_the_lattice_of_1940_pairs(ctx):
    scene = scene_lattice()
    assert len(scene[2]) == 1940 > 1024, "more than 1024 pairs: the finish kernel's threads take more than one each"
    want = _check(ctx, scene, "lattice")
    assert want[2]["touching"] > 1024 and (want[0]["firstPoint"][1:] >= want[0]["firstPoint"][:-1]).all() and want[0]["firstPoint"][-1] > 0


# ---- 7. more jobs than waves -----------------------------------------------------------------------------------------------------------------------

def test_one_pair_with_more_columns_than_the_launch_has_waves(ctx):
    """A 513 x 513 footprint, two voxels high: 263169 jobs for the 2^18 waves of a launch, which take them in turn."""
    rng = np.random.default_rng(17)
    mask = rng.random((513, 513, 2)) > 0.3
    argb = np.where(rng.random((513, 513, 2)) > 0.3, rng.integers(1, 1 << 32, (513, 513, 2), dtype=np.uint64), 0).astype(np.uint32)
    models = [(None, mask), (argb, None)]
    instances = [identity_at((0, 0, 0), (513, 2, 513), 0, FILL), identity_at((0, 0, 0), (513, 2, 513), 1, FILL)]
    want = _check(ctx, (models, instances, np.int32([[0, 1]])), "wide")
    assert want[2]["jobs"] == 513 * 513 > 1 << 18 and want[0]["max"][0].tolist() == [513, 2, 513] and want[2]["points"] > 200000
    last = want[1][want[1]["voxel"][:, 0] == 512]
    assert len(last) > 100 and (last["argbA"] == 0).all() and (last["argbB"] != 0).all(), "points in the columns only a second turn reaches"


# ---- 8. the capacity -------------------------------------------------------------------------------------------------------------------------------

def test_capacities_cut_the_list_and_nothing_else(ctx):
    models, instances, pairs = scene_steps()
    want = model_of(models, instances, pairs)
    total = want[2]["points"]
    p = want[1]
    # a capacity that ends between two points of one job's one step: the first is listed, the second is not
    key = np.stack([p["pair"], p["voxel"][:, 0], p["voxel"][:, 2], (99 - p["voxel"][:, 1]) // 64], axis=1)
    inside = np.nonzero((p["pair"][1:] == 0) & (key[1:] == key[:-1]).all(axis=1))[0]
    assert len(inside) > 10, "pair 0 (X_p's top is y = 99) has steps with several points"
    middle = int(inside[len(inside) // 2]) + 1
    assert (key[middle] == key[middle - 1]).all() and 0 < middle < total
    for capacity in (0, total // 2, middle, total + 5):
        results, points, totals, _ = ctx.model_contacts(models, instances, pairs, capacity=capacity)
        assert results.tobytes() == want[0].tobytes() and totals == want[2] and points.tobytes() == p[:capacity].tobytes(), f"capacity {capacity}"
        got_results, listed, got_totals = _device_call(ctx, models, instances, pairs, capacity, spare=3)
        written = min(capacity, total)
        assert got_results.tobytes() == want[0].tobytes() and got_totals == want[2] and listed[:written].tobytes() == p[:written].tobytes(), f"capacity {capacity} (device)"
        assert (listed[written:].view(np.uint8) == SENTINEL).all(), f"capacity {capacity}: nothing is written beyond the limit"


# ---- 9. no world -----------------------------------------------------------------------------------------------------------------------------------

def test_no_world_is_needed_and_none_is_touched():
    scene = scene_cubes()
    fresh = gpu.Context(0)
    try:
        results, points, totals, _ = fresh.model_contacts(*scene)  # the first call of a context's life
        assert_cubes(results, points, totals)
    finally:
        fresh.close()
    dims = (32, 32, 32)
    solid, colour = flat_world(dims=dims)
    ws = _any_world(dims, solid, colour)
    with_world = gpu.Context(0)
    try:
        with_world.upload_world(ws)
        before = with_world.read_region(0, 0, 0, 32, 32)
        results, points, totals, _ = with_world.model_contacts(*scene)
        assert_cubes(results, points, totals)
        same(_device_call(with_world, *scene, totals["points"]), model_of(*scene), "on a context with a world")
        assert with_world.read_region(0, 0, 0, 32, 32) == before
    finally:
        with_world.close()
        ws.close()


# ---- 10. one statement, three calls ----------------------------------------------------------------------------------------------------------------

def test_it_equals_stamping_b_and_asking_the_world_for_a():
    """For bodies inside an empty world: FILL b with place_models, then cvxc_world_contacts of a with solidOutside = 0 gives this call's overlap,
    sum, pushA (as `normal`), box and, among the points, those with facesB != 0 with facesB as `faces`."""
    dims = (32, 32, 32)
    rng = np.random.default_rng(21)
    models = [random_model(rng, (7, 9, 6), zeros=0.25), cube_model()]
    turned_a = gpu.model_instance(forward_about_centre(rotation(1, 30) @ rotation(0, 15), (7, 9, 6), (22, 21, 23)), (7, 9, 6), 0, FILL)
    turned_b = gpu.model_instance(forward_about_centre(rotation(2, 40), (7, 9, 6), (19, 18, 20)), (7, 9, 6), 0, FILL)
    for name, a, b in (("cubes", identity_at((12, 13, 11), CUBE, 1, FILL), identity_at((10, 10, 10), CUBE, 1, FILL)), ("turned", turned_a, turned_b)):
        instances, pairs = [a, b], np.int32([[0, 1]])
        d = as_dicts(instances)
        assert all(0 <= d[k]["box_min"][i] and d[k]["box_max"][i] <= dims[i] for k in range(2) for i in range(3)), "inside the world"
        assert all(d[0]["box_min"][i] >= d[1]["box_min"][i] for i in range(3)), "origin is a's boxMin: the two sums have one origin"
        want = model_of(models, instances, pairs)
        assert want[0]["overlap"][0] > 0 and (want[1]["facesB"] != 0).any() and (want[0]["pushA"][0] != 0).any()
        empty = np.zeros(dims, dtype=bool)
        ws = _any_world(dims, empty, np.zeros(dims, dtype=np.uint32))
        world = gpu.Context(0)
        try:
            world.upload_world(ws)
            mine, my_points, _, _ = world.model_contacts(models, instances, pairs)
            same((mine, my_points, want[2]), want, name)
            world.place_models(models, [b], 0)
            theirs, their_points, _, _ = world.world_contacts(models, [a], 0)
        finally:
            world.close()
            ws.close()
        r, w = mine[0], theirs[0]
        assert w["overlap"] == r["overlap"] and w["sum"].tolist() == r["sum"].tolist() and w["normal"].tolist() == r["pushA"].tolist(), name
        assert w["origin"].tolist() == r["origin"].tolist() and w["min"].tolist() == r["min"].tolist() and w["max"].tolist() == r["max"].tolist(), name
        listed = my_points[my_points["facesB"] != 0]
        assert len(listed) == len(their_points) == w["points"] > 0 and (listed["voxel"] == their_points["voxel"]).all() and (listed["facesB"] == their_points["faces"]).all(), name
        assert isinstance(their_points, np.ndarray) and their_points.dtype == contactsmodel.POINT_DTYPE


# ---- 11. determinism and errors --------------------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_gives_the_same_bytes(ctx):
    models, instances, pairs = scene_mixed()
    first = ctx.model_contacts(models, instances, pairs)
    second = ctx.model_contacts(models, instances, pairs)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes() and first[2] == second[2] and first[2]["points"] > 0
    total = first[2]["points"]
    one = _device_call(ctx, models, instances, pairs, total)
    two = _device_call(ctx, models, instances, pairs, total)
    assert one[0].tobytes() == two[0].tobytes() == first[0].tobytes() and one[1].tobytes() == two[1].tobytes() == first[1].tobytes()


def test_errors_leave_the_host_arrays_alone_and_set_the_message(ctx):
    models, instances, pairs = scene_cubes()
    descriptors, keep = gpu.Context._models(models, "test")  # noqa: F841
    inst = gpu.Context._instances(instances)
    results = np.full(2, SENTINEL, dtype=np.uint8).repeat(RESULT_BYTES)
    points = np.full(4 * POINT_BYTES, SENTINEL, dtype=np.uint8)

    def raw(entry=None, models_ptr=True, model_count=1, instance_list=inst, pair_array=pairs, results_ptr=True, points_ptr=True, capacity=4):
        p = np.ascontiguousarray(pair_array, dtype=np.int32).reshape(-1, 2)
        summary, ms = gpu.PairsSummary(), gpu.C.c_float()
        ctx._check((entry or gpu.lib().cvxp_model_contacts)(
            ctx._h, gpu.C.addressof(descriptors) if models_ptr else None, model_count, gpu.C.addressof(instance_list), len(instance_list), p.ctypes.data if len(p) else None,
            len(p), results.ctypes.data if results_ptr else None, points.ctypes.data if points_ptr else None, capacity, gpu.C.byref(summary), gpu.C.byref(ms)))

    far = identity_at((10, 13, 10), CUBE, 0, FILL)
    far.boxMax[2] = (1 << 30) + 1
    big_m = identity_at((10, 13, 10), CUBE, 0, FILL)
    big_m.toModel.m[0][0] = (1 << 24) + 1
    wide = identity_at((0, 0, 0), CUBE, 0, FILL)
    wide.boxMin[0] = wide.boxMin[2] = -(1 << 15)
    wide.boxMax[0] = wide.boxMax[2] = 1 << 15
    for kwargs, message in (
            (dict(models_ptr=False), "cvxp_model_contacts: models NULL or modelCount 1"), (dict(model_count=257), "modelCount 257 outside 1 .. 256"),
            (dict(instance_list=gpu.Context._instances([instances[0], identity_at((0, 0, 0), CUBE, 3, FILL)])), "instance 1: model 3 outside 0 .. 0"),
            (dict(instance_list=gpu.Context._instances([far, instances[1]])), r"instance 0: the box \[10, 1073741825\) on axis 2 has a coordinate beyond 2\^30"),
            (dict(instance_list=gpu.Context._instances([instances[0], big_m])), r"instance 1: toModel: m\[0\]\[0\]"),
            (dict(pair_array=np.zeros((0, 2), dtype=np.int32)), "pairs NULL or pairCount 0 outside 1 .. 65536"),
            (dict(pair_array=np.zeros((65537, 2), dtype=np.int32) + [0, 1]), "pairCount 65537 outside 1 .. 65536"),
            (dict(pair_array=[[0, 1], [1, 2]]), r"pair 1: \(1, 2\) has an index outside 0 .. 1"), (dict(pair_array=[[-1, 1]]), r"pair 0: \(-1, 1\) has an index outside"),
            (dict(pair_array=[[0, 1], [0, 1], [1, 1]]), r"pair 2: \(1, 1\) pairs an instance with itself"), (dict(results_ptr=False), "results is NULL"),
            (dict(capacity=-1), "pointCapacity -1 with a list"), (dict(points_ptr=False), "pointCapacity 4 with no list"),
            (dict(entry=gpu.lib().cvxp_model_contacts_device, results_ptr=False), "cvxp_model_contacts_device: results is NULL"),
            (dict(instance_list=gpu.Context._instances([wide, wide])), "error -4: cvxp_model_contacts: the pairs' common footprints sum to")):
        with pytest.raises(gpu.CvxError, match=message):
            raw(**kwargs)
        assert (results == SENTINEL).all() and (points == SENTINEL).all(), message
    with pytest.raises(gpu.CvxError, match="model 0: argb and solid are both NULL"):
        ctx.model_contacts_device([(CUBE, 0, 0)], instances, pairs, torch.zeros(2 * RESULT_BYTES, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="at least 2 x 144 bytes"):
        ctx.model_contacts_device([(CUBE, 0, 0)], instances, pairs, torch.zeros(RESULT_BYTES, dtype=torch.uint8, device="cuda"))
    got = ctx.model_contacts(models, instances, pairs)
    assert_cubes(got[0], got[1], got[2])
    raw()  # the same arrays take a good call
    assert results.view(gpu.PAIR_RESULT_DTYPE).tobytes() == got[0].tobytes() and points.view(gpu.PAIR_POINT_DTYPE).tobytes() == got[1][:4].tobytes()
