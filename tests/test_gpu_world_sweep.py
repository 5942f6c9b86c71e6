"""GPU: cvxs_world_sweep / cvxs_world_sweep_device (include/cpuvox_gpu_sweep.h) against the numpy model of tests/sweepmodel.py -- sweeps,
contacts, points and summary byte for byte -- and against the shipped cvxc_world_contacts composed a pose at a time: no overlap at any
instance_moved(I, o_j) with j < hit, the contacts' bytes at hit.  The cases are tests/sweepcases.py's, the ones tests/test_world_sweep_cpu.py
runs through the host rules; each first asserts from the model the property it is named for.  Everything is integers: no tolerance."""
import numpy as np
import pytest
import torch

import pickmodel
import sweepcases
import sweepmodel
from cpuvox_amd import gpu
from test_gpu_world_contacts import SENTINEL, World, _device_models
from test_world_contacts_cpu import colour_of
from test_world_models_cpu import identity_at
from test_world_sweep_cpu import property_of, same

pytestmark = pytest.mark.gpu

DEFAULT = gpu.SURFACE_OUTSIDE_DEFAULT


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(key):
        if key not in made:
            made[key] = World(*sweepcases.world(key))
        return made[key]
    yield get
    for w in made.values():
        w.close()


def _composed(ctx, models, instances, motions, so, sweeps, contacts):
    """The shipped world_contacts on instance_moved(I, o_j): overlap 0 for every j < hit (every j when hit is -1), the sweep's contacts at hit."""
    before = []
    for inst, v, s in zip(instances, motions, sweeps):
        path = sweepmodel.path(v)
        assert (list(path[s["hit"]][0]) if s["hit"] >= 0 else list(v)) == s["at"].tolist()
        before += [gpu.instance_moved(inst, o) for o, _ in path[:s["hit"] if s["hit"] >= 0 else len(path)]]
    for at in range(0, len(before), gpu.MODELS_MAX_INSTANCES):
        results, _, totals, _ = ctx.world_contacts(models, before[at:at + gpu.MODELS_MAX_INSTANCES], so, capacity=0)
        assert totals["overlap"] == 0 and not results["overlap"].any(), "a pose before `hit` overlaps the world"
    touching = [gpu.instance_moved(inst, s["at"]) for inst, s in zip(instances, sweeps)]
    results, points, totals, _ = ctx.world_contacts(models, touching, so)
    assert results.tobytes() == contacts.tobytes(), "the contacts are cvxc_world_contacts' of the moved instances"
    assert ((results["overlap"] > 0) == (sweeps["hit"] >= 0)).all()
    return points


def _device_call(ctx, models, instances, motions, so, capacity, spare=2):
    """One device call into sentinel-filled tensors -> (sweeps, contacts, the points tensor's entries, totals)."""
    descriptors, keep = _device_models(models)  # noqa: F841
    contacts = torch.full((len(instances) * 120,), SENTINEL, dtype=torch.uint8, device="cuda")
    points = torch.full(((capacity + spare) * 24,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sweeps, totals, ms = ctx.world_sweep_device(descriptors, instances, motions, contacts, points[:capacity * 24] if capacity else None, so)
    assert ms > 0.0
    return sweeps, contacts.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE), points.cpu().numpy().view(gpu.CONTACT_POINT_DTYPE), totals


def _check(worlds, name, device=True):
    """The host call against the model and the composed contacts calls, then the device call against the model."""
    property_of(name)
    key, models, instances, motions, so = sweepcases.case(name)
    want = sweepcases.answer(name)
    ctx = worlds(key).ctx
    sweeps, contacts, points, totals, ms = ctx.world_sweep(models, instances, motions, so)
    assert ms > 0.0
    same((sweeps, contacts, points, totals), want, name)
    listed = _composed(ctx, models, instances, motions, so, sweeps, contacts)
    assert listed.tobytes() == points.tobytes()
    if device:
        n = want[3]["points"]
        got = _device_call(ctx, models, instances, motions, so, n)
        same((got[0], got[1], got[2][:n], got[3]), want, name + " (device)")
        assert (got[2][n:].view(np.uint8) == SENTINEL).all(), "entries beyond the capacity keep what they held"
    return want


# ---- 1. the thin shell and the ends of the range --------------------------------------------------------------------------------------------------------

def test_a_plate_falling_through_a_thin_floor_is_caught(worlds):
    key, models, instances, motions, so = sweepcases.case("thin shell")
    ctx = worlds(key).ctx
    ends = [instances[0], gpu.instance_moved(instances[0], motions[0])]
    results, _, totals, _ = ctx.world_contacts(models, ends, so, capacity=0)
    assert results["overlap"].tolist() == [0, 0] and totals["touching"] == 0, "cvxc_world_contacts sees nothing at either end pose"
    want = _check(worlds, "thin shell")
    assert (want[0]["hit"][0], want[0]["axis"][0], want[0]["sign"][0]) == (5, 1, -1)


@pytest.mark.parametrize("name", ["starts solid", "hit at n", "miss by one", "still"])
def test_the_ends_of_the_range(worlds, name):
    _check(worlds, name)


# ---- 2. axes, signs, ties and the outside ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["-x", "+x", "+x open", "-y", "+y", "-z", "+z", "3 -1 2", "2 2 2", "-5 7 -3"])
def test_every_axis_and_sign_and_the_tie_order(worlds, name):
    _check(worlds, name)


@pytest.mark.parametrize("name", ["below the world", "sideways", "sideways open"])
def test_outside_the_world(worlds, name):
    _check(worlds, name)


# ---- 3. waves and the binary search ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["column 65", "column 200", "column 300", "lane 0", "lane 63"])
def test_steps_and_lanes_of_a_wave(worlds, name):
    _check(worlds, name)


def test_the_binary_search_over_a_column_of_40_runs(worlds):
    _check(worlds, "comb")


def test_rotated_and_scaled_maps_on_the_terrain(worlds):
    _check(worlds, "maps")


# ---- 4. many jobs ---------------------------------------------------------------------------------------------------------------------------------------

def test_many_instances_many_stations_and_the_order_of_the_instances(worlds):
    _check(worlds, "65 instances")
    want = _check(worlds, "4096 instances")
    key, models, instances, motions, so = sweepcases.case("4096 instances")
    ctx = worlds(key).ctx
    # the same call twice: the same bytes; reversed: the same bytes per instance (but for firstPoint, the list's order)
    again = ctx.world_sweep(models, instances, motions, so)
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes() and again[2].tobytes() == want[2].tobytes() and again[3] == want[3]
    back = ctx.world_sweep(models, instances[::-1], motions[::-1], so, point_capacity=0)
    assert back[0][::-1].tobytes() == want[0].tobytes()
    mine, theirs = back[1][::-1].copy(), want[1].copy()
    mine["firstPoint"] = theirs["firstPoint"] = 0
    assert mine.tobytes() == theirs.tobytes() and back[3] == want[3]
    # the longest motion, then a small call
    _check(worlds, "8193 stations")
    _check(worlds, "65 instances", device=False)


def test_the_sweeps_alone(worlds):
    """contacts NULL: the sweeps and the summary without points."""
    key, models, instances, motions, so = sweepcases.case("maps")
    want = sweepcases.answer("maps")
    descriptors, keep = _device_models(models)  # noqa: F841
    sweeps, totals, ms = worlds(key).ctx.world_sweep_device(descriptors, instances, motions, None, None, so)
    assert sweeps.tobytes() == want[0].tobytes() and totals == dict(want[3], points=0) and ms > 0.0


# ---- 5. the flight loop ---------------------------------------------------------------------------------------------------------------------------------

def test_a_lifted_piece_is_swept_down_to_rest_and_filled():
    dims = (32, 64, 32)
    solid = np.zeros(dims, dtype=bool)
    solid[:, :8, :] = True
    solid[10:18, 8:30, 12:20] = True  # a pillar on the ground ...
    solid[8:20, 30:36, 10:22] = True  # ... with a wider head
    colour = colour_of(solid)
    neck = [{"op": gpu.BRUSH_CARVE, "shape": 0, "a": (0, 18, 0), "b": (32, 28, 32), "argb": 0}]
    world = World(dims, solid.copy(), colour.copy())
    try:
        ctx = world.ctx
        ctx.brush(neck, 5)
        pickmodel.apply_strokes(world.solid, world.colour, neck)
        argb = torch.zeros(4096, dtype=torch.int32, device="cuda")
        mask = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pieces, summary, _ = ctx.world_lift_pieces_device((0, 0, 0), dims, gpu.ANCHOR_GROUND, argb, mask, gpu.LIFT_REMOVE, 5, 16, 4096)
        assert len(pieces) == 1 and pieces[0]["piece"]["min"].tolist() == [8, 28, 10]
        lifted = gpu.lifted_model(pieces, 0, argb.data_ptr(), mask.data_ptr())
        size = lifted[0]
        assert size == (12, 8, 12)
        body = identity_at((8, 28, 10), size, 0, gpu.BRUSH_FILL)
        velocity = (3, -30, 0)  # the piece's core, the pillar's two layers y = 28, 29 below the head, comes down on the stump's top, y = 17
        contacts = torch.zeros(120, dtype=torch.uint8, device="cuda")
        sweeps, totals, ms = ctx.world_sweep_device([lifted], [body], [velocity], contacts, None, DEFAULT)
        s = sweeps[0]
        assert ms > 0.0 and totals["hits"] == 1 and (s["axis"], s["sign"]) == (1, -1)
        assert s["free"].tolist() == [1, 18 - 28, 0] and s["at"].tolist() == [1, 17 - 28, 0], "x has made the one step it makes before y's sixth"
        path = sweepmodel.path(velocity)
        assert path[s["hit"] - 1][0] == tuple(s["free"]) and path[s["hit"]][0] == tuple(s["at"])
        rest, further = gpu.instance_moved(body, s["free"]), gpu.instance_moved(body, s["at"])
        both = torch.zeros(240, dtype=torch.uint8, device="cuda")
        ctx.world_contacts_device([lifted], [rest, further], both)
        both = both.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE)
        assert both["overlap"][0] == 0 and both["overlap"][1] > 0, "free at `free`, touching one step further along the path"
        assert contacts.cpu().numpy().tobytes() == both[1:2].tobytes(), "the sweep's contacts are those of the touching pose"
        ctx.place_models_device([lifted], [rest], 5)
        after = torch.zeros(120, dtype=torch.uint8, device="cuda")
        ctx.world_contacts_device([lifted], [rest], after)
        after = after.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE)[0]
        assert after["overlap"] == after["voxels"] > 0, "the FILL made the body's voxels solid where it came to rest"
    finally:
        world.close()
