"""GPU: travel-distance fields through the air or the solid of the device-resident world (cvx_world_spread[_device]).

Every field and its totals are compared with the independent dense model of tests/spreadmodel.py; everything is integers and no comparison has a
tolerance.  The worlds are those of the other world calls' tests -- the 128 x 64 x 128 terrain and the 32 x 256 x 32 tall world -- and purpose-built
ones; shapes are derived from T = gpu.SPREAD_TILE, the tile a workgroup relaxes.  Every case asserts from the model that its input has the property
it is named for before it calls the device."""
import ctypes as C

import numpy as np
import pytest

import pickmodel
import spreadmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _dense, _world
from test_gpu_world_dense import TALL, _any_world, _tall_solid
from test_gpu_world_edit import DIMS, _terrain
from test_world_spread_cpu import AIR, BLOCKED, MASKS, SOLID, TOTALS, UNREACHED, seeds_of, serpentine, world_of

pytestmark = pytest.mark.gpu
T = gpu.SPREAD_TILE


@pytest.fixture(scope="module")
def terrain():
    solid = _terrain()
    ws = _world(solid, _dense(solid))
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    yield DIMS, solid, ctx
    ctx.close()
    ws.close()


@pytest.fixture(scope="module")
def tall():
    solid = _tall_solid()
    ws = _any_world(TALL, solid, _dense(solid))
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    yield TALL, solid, ctx
    ctx.close()
    ws.close()


def _open(solid):
    ws = world_of(solid)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    return ctx, ws


def _check(ctx, solid, lo, hi, seeds, medium, mask, cut, label=""):
    """One call against the model: the field, the totals, the bound on the launches.  Returns (field, summary, the model's summary)."""
    want, expected = spreadmodel.field(solid, lo, hi, seeds, medium, mask, cut)
    got, summary, ms = ctx.world_spread(lo, hi, seeds, medium=medium, step_faces=mask, max_steps=cut)
    assert got.shape == want.shape and got.dtype == np.int32
    bad = got != want
    assert not bad.any(), f"{label} medium {medium} mask {mask:#x} box {lo} .. {hi} cut {cut}: {int(bad.sum())} of {bad.size} differ, first at " \
                          f"{np.argwhere(bad)[0].tolist()} (x, z, y): {got[bad][0]} for {want[bad][0]}"
    assert {k: summary[k] for k in TOTALS} == {k: expected[k] for k in TOTALS}, (label, summary, expected)
    assert 1 <= summary["launches"] <= cut + 2 and summary["tileVisits"] >= 0 and ms > 0.0
    return got, summary, expected


# ---- 1. both media, every mask, 1 / 7 / 4096 seeds, host array and device tensor ---------------------------------------------------------------------

@pytest.mark.parametrize("world_name", ["terrain", "tall"])
@pytest.mark.parametrize("medium", [AIR, SOLID])
@pytest.mark.parametrize("mask_name", sorted(MASKS))
def test_fields_equal_the_model(terrain, tall, world_name, medium, mask_name):
    import torch

    dims, solid, ctx = terrain if world_name == "terrain" else tall
    mask = MASKS[mask_name]
    lo, hi = ((-3, -2, 50), (67, 45, 131)) if world_name == "terrain" else ((-2, -2, -2), (34, 258, 34))
    rng = np.random.default_rng(100 * medium + mask)
    reached = 0
    on_medium = np.argwhere(spreadmodel.passable(solid, lo, hi, medium))
    for count in (1, 7, 4096):
        seeds = seeds_of(rng, dims, count, 5)
        for k, (x, z, y) in enumerate(on_medium[rng.integers(0, len(on_medium), min(count, 3))]):  # on the medium, whatever the dice say
            seeds[k] = (int(x) + lo[0], int(y) + lo[1], int(z) + lo[2], 2 * k)
        if count > 1:
            seeds[3] = (lo[0] - 1, lo[1], lo[2], 0)  # ... and one outside the box
        got, summary, expected = _check(ctx, solid, lo, hi, seeds, medium, mask, 90, f"{world_name}, {count} seeds")
        assert 0 < expected["seedsUsed"] and (count == 1 or expected["seedsUsed"] < count), "seeds on and off the medium"
        reached += expected["reached"]
        if count == 7:  # the device form: the same bytes in a torch tensor
            out = torch.full(got.shape, 12345, dtype=torch.int32, device="cuda")
            summary_d, ms = ctx.world_spread_device(lo, hi, seeds, out, medium=medium, step_faces=mask, max_steps=90)
            assert out.cpu().numpy().tobytes() == got.tobytes() and ms > 0.0
            assert {k: summary_d[k] for k in TOTALS} == {k: summary[k] for k in TOTALS}
            again, _, _ = ctx.world_spread(lo, hi, list(reversed(seeds)), medium=medium, step_faces=mask, max_steps=90)
            assert again.tobytes() == got.tobytes(), "no seed order shows"
    assert reached > 1000


# ---- 2. box extents ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_box_extents_around_the_tile(tall, axis):
    dims, solid, ctx = tall
    for size in (1, T[axis] - 1, T[axis], T[axis] + 1, 2 * T[axis] + 1):
        for medium in (AIR, SOLID):
            lo = [3, 15, 2]  # (y = 15: the terrain's top, both media in every layer)
            hi = [3 + 11, 15 + 70, 2 + 13]
            hi[axis] = lo[axis] + size
            ok = spreadmodel.passable(solid, lo, hi, medium)
            assert ok.any(), (axis, size, medium)
            x, z, y = np.argwhere(ok)[len(np.argwhere(ok)) // 2]
            _check(ctx, solid, tuple(lo), tuple(hi), [(int(x) + lo[0], int(y) + lo[1], int(z) + lo[2])], medium, 0x3F, 300, f"axis {axis} size {size}")


def test_boxes_on_across_and_outside_the_world(terrain):
    dims, solid, ctx = terrain
    assert not solid[40, 30, 40] and solid[40, 2, 40]
    got, summary, _ = _check(ctx, solid, (40, 30, 40), (41, 31, 41), [(40, 30, 40, 3)], AIR, 0x3F, 9, "1 x 1 x 1 on a seed")
    assert got.tolist() == [[[3]]] and summary["launches"] == 1
    sides = {"-x": ((-5, 40, 40), (6, 50, 50)), "+x": ((120, 40, 40), (133, 50, 50)), "-y": ((40, -4, 40), (50, 30, 50)), "+y": ((40, 50, 40), (50, 70, 50)),
             "-z": ((40, 40, -7), (50, 50, 4)), "+z": ((40, 40, 125), (50, 50, 140))}
    for name, (lo, hi) in sides.items():
        inside = [min(max(lo[a], 0), dims[a] - 1) for a in range(3)]
        medium = SOLID if name == "-y" else AIR
        got, _, expected = _check(ctx, solid, lo, hi, [tuple(inside)], medium, 0x3F, 40, name)
        outside = np.ones(got.shape, dtype=bool)
        outside[max(-lo[0], 0):dims[0] - lo[0], max(-lo[2], 0):dims[2] - lo[2], max(-lo[1], 0):dims[1] - lo[1]] = False
        assert outside.any() and (got[outside] == BLOCKED).all() and expected["reached"] > 0, name
    for lo, hi in (((-20, 0, 0), (-9, 5, 5)), ((0, 64, 0), (9, 70, 9)), ((0, -9, 0), (5, 0, 5)), ((128, 0, 128), (130, 3, 131))):
        got, summary, _ = _check(ctx, solid, lo, hi, [lo, (5, 5, 5)], AIR, 0x3F, 5, "wholly outside")
        assert (got == BLOCKED).all() and {k: summary[k] for k in TOTALS} == {"passable": 0, "reached": 0, "largestDistance": -1, "seedsUsed": 0}


# ---- 3. the detour ------------------------------------------------------------------------------------------------------------------------------------------

def test_a_tile_is_lowered_again_when_the_short_way_arrives_through_the_neighbour():
    tx = T[0]
    assert tx >= 8 and T[2] >= 5
    solid = np.ones((32, 64, 32), dtype=bool)
    # y = 2: seed S = (tx - 2, 2, 0); the short way to V = (tx - 1, 2, 2) leaves the tile: (tx - 1, 0), (tx, 0), (tx, 1), (tx, 2), V;
    # the long way stays inside it: along z = 0 to x = 0, up to z = 4, along z = 4 to x = tx - 1, down to V; beyond V the row z = 2 goes on to x = 2
    solid[0:tx + 1, 2, 0] = False
    solid[tx, 2, 0:3] = False
    solid[2:tx + 1, 2, 2] = False
    solid[0, 2, 0:5] = False
    solid[0:tx, 2, 4] = False
    solid[tx - 1, 2, 2:5] = False
    # y = 10: a U that leaves the tile and comes back, nothing else
    solid[tx - 3:tx + 1, 10, 0] = False
    solid[tx, 10, 0:3] = False
    solid[tx - 3:tx + 1, 10, 2] = False
    lo, hi = (0, 0, 0), (32, 64, 32)
    seeds = [(tx - 2, 2, 0), (tx - 3, 10, 0)]
    whole, _ = spreadmodel.field(solid, lo, hi, seeds, AIR, 0x3F, 1000)
    alone, _ = spreadmodel.field(solid, lo, (tx, T[1], T[2]), seeds, AIR, 0x3F, 1000)  # the seeds' tile with nothing around it
    assert whole[tx - 1, 2, 2] == 5 and alone[tx - 1, 2, 2] == (tx - 2) + 4 + (tx - 1) + 2 > 5, "V: first the long way inside its tile, then the short one"
    assert whole[2, 2, 2] == 5 + tx - 3 and alone[2, 2, 2] > whole[2, 2, 2], "... and what lies behind V falls with it"
    assert whole[tx - 3, 2, 10] == 3 + 2 + 3 and alone[tx - 3, 2, 10] == UNREACHED, "the only way leaves the tile and comes back"
    ctx, ws = _open(solid)
    try:
        _, summary, _ = _check(ctx, solid, lo, hi, seeds, AIR, 0x3F, 1000, "detour")
        assert summary["launches"] >= 3
    finally:
        ctx.close()
        ws.close()


# ---- 4. ties, starts, duplicates, ignored seeds ----------------------------------------------------------------------------------------------------------

def test_ties_starts_duplicates_and_ignored_seeds(terrain):
    dims, solid, ctx = terrain
    lo, hi = (0, 0, 0), DIMS
    air = ~solid[:, 44:48, :]
    assert air.all(), "open air above the slabs"
    a, b = (2 * T[0] + 1, 45, 20), (6 * T[0] + 3, 45, 20)
    middle = ((a[0] + b[0]) // 2, 45, 20)
    assert a[0] // T[0] != b[0] // T[0] != middle[0] // T[0] and middle[0] - a[0] == b[0] - middle[0]
    loser, winner = (90, 45, 90, 30), (100, 45, 90, 0)
    ignored = [(10, 0, 10, 0), (-1, 45, 20, 0), (50, 64, 50, 0), (128, 45, 128, 0)]
    assert solid[10, 0, 10]
    seeds = [a + (0,), b + (0,), loser, winner, (60, 46, 100, 7), (60, 46, 100, 2), (60, 46, 100, 4)] + ignored
    want, expected = spreadmodel.field(solid, lo, hi, seeds, AIR, 0x3F, 200)
    assert want[middle[0], middle[2], middle[1]] == middle[0] - a[0], "two seeds in different tiles tie"
    assert want[loser[0], loser[2], loser[1]] == 10 < loser[3], "a farther seed with start 0 wins"
    assert want[60, 100, 46] == 2 and expected["seedsUsed"] == len(seeds) - len(ignored) == 7
    _check(ctx, solid, lo, hi, seeds, AIR, 0x3F, 200, "ties")


# ---- 5. the cut ---------------------------------------------------------------------------------------------------------------------------------------------

def test_the_cut(terrain):
    dims, solid, ctx = terrain
    lo, hi = (16, 40, 16), (16 + 3 * T[0], 50, 16 + 3 * T[2])
    seed = (lo[0] + T[0] - 5, 44, lo[2] + 3)
    assert not solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].any()
    got, summary, _ = _check(ctx, solid, lo, hi, [seed], AIR, 0x3F, 1, "maxSteps 1")
    assert summary["reached"] == 7 and summary["largestDistance"] == 1 and int((got == UNREACHED).sum()) == got.size - 7
    got, summary, _ = _check(ctx, solid, lo, hi, [seed], AIR, 0x3F, 4, "the cut on a tile face")
    row = got[:, seed[2] - lo[2], seed[1] - lo[1]]
    assert row[T[0] - 1] == 4 and row[T[0]] == UNREACHED and summary["largestDistance"] == 4, "D == maxSteps on the tile's last voxel, maxSteps + 1 beyond the face"
    got, _, _ = _check(ctx, solid, lo, hi, [seed + (4,)], AIR, 0x3F, 4, "start == maxSteps")
    assert int((got >= 0).sum()) == 1


# ---- 6. the long corridor --------------------------------------------------------------------------------------------------------------------------------

def test_the_long_corridor():
    solid, cells = serpentine()
    lo, hi = (0, 0, 0), (64, 64, 64)
    want, _ = spreadmodel.field(solid, lo, hi, [cells[0] + (0,)], AIR, 0x3F, 65534)
    assert int((want > 32767).sum()) == 32767 and int((want == 65534).sum()) == 1, "values a signed 16-bit reading would spoil"
    c = np.array(cells[-1024:])
    assert (want[c[:, 0], c[:, 2], c[:, 1]] == UNREACHED).all() and int((want == UNREACHED).sum()) == 1024
    ctx, ws = _open(solid)
    try:
        _, summary, _ = _check(ctx, solid, lo, hi, [cells[0] + (0,)], AIR, 0x3F, 65534, "corridor")
        assert summary["launches"] <= 65536 and summary["largestDistance"] == 65534
        assert solid[1, 1, 1]
        _, _, expected = _check(ctx, solid, lo, hi, [(1, 1, 1)], SOLID, 0x3F, 65534, "around the corridor")
        assert expected["passable"] == 64 ** 3 - 66559 == expected["reached"], "one blocked corridor, everything around it passable"
    finally:
        ctx.close()
        ws.close()


# ---- 7. the work list -----------------------------------------------------------------------------------------------------------------------------------

def test_a_sealed_room_costs_its_own_tiles():
    solid = np.ones((64, 64, 64), dtype=bool)
    x0, z0 = 2 * T[0] + 1, 3 * T[2] + 1
    solid[x0:x0 + T[0] - 2, 20:40, z0:z0 + T[2] - 2] = False  # inside one tile, walls all around
    lo, hi = (0, 0, 0), (64, 64, 64)
    tiles = -(-64 // T[0]) * -(-64 // T[1]) * -(-64 // T[2])
    assert tiles >= 64 and x0 // T[0] == (x0 + T[0] - 3) // T[0] and z0 // T[2] == (z0 + T[2] - 3) // T[2]
    ctx, ws = _open(solid)
    try:
        _, summary, expected = _check(ctx, solid, lo, hi, [(x0, 20, z0)], AIR, 0x3F, 500, "sealed room")
        assert expected["reached"] == expected["passable"] == (T[0] - 2) * 20 * (T[2] - 2)
        assert 0 < summary["tileVisits"] < tiles * summary["launches"], summary
    finally:
        ctx.close()
        ws.close()


# ---- 8. the pond ------------------------------------------------------------------------------------------------------------------------------------------

def test_the_pond_fills_and_a_carved_wall_lets_it_run_on():
    import torch

    solid = _terrain()
    colour = _dense(solid)
    level = 13
    lo, hi = (0, 0, 0), (96, level, 96)  # the box's top is the water level
    open_top = np.argwhere(~solid[:96, level - 1, :96])
    assert len(open_top) > 50
    sx, sz = (int(v) for v in open_top[len(open_top) // 3])
    spring = (sx, level - 1, sz)
    first, expected = spreadmodel.field(solid, lo, hi, [spring], AIR, 0x37, 4000)
    assert 100 < expected["reached"] < expected["passable"], "a pond, not the whole box: other basins stay dry"
    ws = _world(solid, colour)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    try:
        out = torch.zeros(first.shape, dtype=torch.int32, device="cuda")
        summary, _ = ctx.world_spread_device(lo, hi, [spring], out, medium=AIR, step_faces=0x37, max_steps=4000)
        assert out.cpu().numpy().tobytes() == first.tobytes() and summary["reached"] == expected["reached"]
        water = torch.where(out >= 0, 1, 0).to(torch.uint8).contiguous()
        argb = torch.full(first.shape, 0xFF2040C0 - (1 << 32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.write_voxels_device(lo, hi, argb.data_ptr(), water.data_ptr(), op=gpu.BRUSH_FILL)
        filled = solid.copy()
        filled[:96, :level, :96] |= (first >= 0).transpose(0, 2, 1)
        assert (ctx.read_voxels((0, 0, 0), DIMS, want_argb=False)[1] == filled.transpose(0, 2, 1)).all()
        # a trench through land and water; the next spread starts behind the call that dug it and reads what it left
        stroke = [{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_BOX, "a": (10, 6, sz - 1), "b": (90, level + 3, sz + 1), "argb": 0}]
        dug, dug_colour = filled.copy(), np.where(filled, np.uint32(1), np.uint32(0))
        pickmodel.apply_strokes(dug, dug_colour, gpu.strokes_array(stroke))
        assert (dug != filled).any() and (dug & ~solid)[:96, :level, :96].any(), "the trench cuts land; some water remains beside it"
        ctx.brush(stroke)
        second, expected2 = spreadmodel.field(dug, lo, hi, [spring], AIR, 0x37, 4000)
        assert not dug[spring] and (second != first).any() and expected2["reached"] > 0
        got, summary2, _ = ctx.world_spread(lo, hi, [spring], medium=AIR, step_faces=0x37, max_steps=4000)
        assert (got == second).all() and summary2["reached"] == expected2["reached"]
    finally:
        ctx.close()
        ws.close()


# ---- 9. a repeating world does not wrap; bad arguments ---------------------------------------------------------------------------------------------------

def test_a_repeating_world_does_not_wrap_and_bad_arguments_leave_out_alone(terrain):
    dims, solid, ctx = terrain
    lo, hi = (-10, 40, -10), (12, 50, 12)
    ctx.set_world_repeat(True)
    try:
        got, _, _ = _check(ctx, solid, lo, hi, [(0, 45, 0), (-3, 45, -3)], AIR, 0x3F, 50, "repeat")
        assert (got[:10] == BLOCKED).all() and (got[:, :10] == BLOCKED).all() and (got[10:, 10:] >= 0).all()
    finally:
        ctx.set_world_repeat(False)
    L = gpu.lib()
    out = np.full(8, 7, dtype=np.int32)
    seed = gpu.seeds_array([(0, 45, 0)])
    summary = gpu.SpreadSummary(1, 2, 3, 4, 5, 6, 7)

    def call(fn=L.cvx_world_spread, handle=None, seeds=seed, count=1, target=out, **changes):
        p = gpu.SpreadParams((C.c_int32 * 3)(0, 44, 0), (C.c_int32 * 3)(2, 46, 2), AIR, 0x3F, 10, 0)
        for name, value in changes.items():
            setattr(p, name, value)
        return fn(handle or ctx._h, C.addressof(p), seeds.ctypes.data if seeds is not None else None, count, target.ctypes.data if target is not None else None,
                  C.addressof(summary), None)

    bad = [call(medium=2), call(stepFaces=0), call(stepFaces=0x7F), call(maxSteps=0), call(maxSteps=65535), call(count=0), call(count=4097),
           call(seeds=None), call(target=None), call(boxMax=(C.c_int32 * 3)(2, 44, 2)), call(boxMin=(C.c_int32 * 3)(0, 44, -(1 << 30) - 1)),
           call(seeds=gpu.seeds_array([(0, 45, 0, 11)])), call(fn=L.cvx_world_spread_device, seeds=gpu.seeds_array([(0, 45, 0, -1)]))]
    assert bad == [-1] * len(bad) and (out == 7).all() and summary.tileVisits == 7 and summary.passable == 1
    with pytest.raises(gpu.CvxError, match="seed 1: start 11 outside 0 .. maxSteps 10"):
        ctx.world_spread((0, 44, 0), (2, 46, 2), [(0, 45, 0), (0, 45, 0, 11)], medium=AIR, max_steps=10)
    empty = gpu.Context(0)
    try:
        assert call(handle=empty._h) == -3 and (out == 7).all()  # CVX_ERR_NOT_READY
    finally:
        empty.close()
    assert call() == 0 and (out >= 0).all() and summary.reached == 8
