"""GPU: walking-distance fields on the device-resident world (cvx_world_nav_build, cvx_nav_field_goals, cvx_nav_query, cvx_nav_query_device).

Every comparison with the dense model of tests/navmodel.py is exact: all 32 bytes of the cvx_nav_step of EVERY voxel position of the world (one
query), plus the deterministic fields of the summary; every build is made twice with identical query bytes.

The noise worlds draw noise_world's generator at NOISE_DENSITY[dims, width] (tests/test_world_nav_cpu.py): 70 % solid leaves no standing room
for a body wider than a voxel.  The densities were chosen on the CPU so that the model ALONE, for the rule height 2, stepUp 1, maxDrop 3 and the
three goals of noise_goals, satisfies the preconditions test_noise_worlds asserts first -- reached nodes in at least 100 columns, at least 20
columns with two or more reached nodes, a node that exists but is unreached, largestDistance at least twice the solve kernel's tile width
(2 * 16).  The model's counts (nodes, reached, largestDistance, columns with a reached node, columns with two or more):
  (32, 32, 32)  width 1 density 0.30: 5279  763 43 519 199      (16, 64, 32)  width 1 density 0.25: 4846 1349 55 480 408
                width 2 density 0.08: 4887 1475 43 858 495                    width 2 density 0.10: 4508 2632 74 465 464
                width 3 density 0.03: 4338 2860 78 896 841                    width 3 density 0.05: 4037 1766 56 420 419
No test asserts a time.  A relax loop that does not settle ends in an error return after nodes + 2 launches: no test can spin."""
import ctypes as C

import numpy as np
import pytest

import navmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _box
from test_gpu_world_edit import DIMS
from test_gpu_world_pieces import built  # noqa: F401  (the fixture: the floor at y = 0 plus strokes, on the device and in numpy)
from test_world_brush_cpu import _pick_world
from test_world_nav_cpu import NOISE_DENSITY, NOISE_DIMS, RULES, nav_noise_world, noise_goals, random_call, walk, walk_starts, world_calls

pytestmark = pytest.mark.gpu

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
ROCK = 0xFF808080
TILE = 16            # nav_relax_kernel's tile width (cpuvox_amd/csrc/cvx_nav.hip, kTile)
TILE_NODES = 1536    # ... and the nodes a tile may hold in LDS (kTileNodes)
_POSITIONS = {}


def _positions(dims):
    """Every voxel position of a world of `dims`, in (x, y, z) order."""
    if dims not in _POSITIONS:
        _POSITIONS[dims] = np.ascontiguousarray(np.indices(dims, dtype=np.int32).reshape(3, -1).T)
    return _POSITIONS[dims]


def _field(ctx, solid, call, goals, label=""):
    """Builds the field twice (identical query bytes) and compares the query of every voxel position and the summary with the model.
    -> (the open field, the model's steps[x, y, z], the model's summary)."""
    box_min, box_max, width, height, step_up, max_drop, max_steps = call
    dims = tuple(solid.shape)
    want, want_summary = navmodel.analyse(solid, box_min, box_max, width, height, step_up, max_drop, goals, max_steps)
    kw = dict(width=width, height=height, step_up=step_up, max_drop=max_drop, max_steps=max_steps)
    field = ctx.nav_build(box_min, box_max, goals, **kw)
    try:
        got = field.query(_positions(dims))
        again = ctx.nav_build(box_min, box_max, goals, **kw)
        try:
            assert again.query(_positions(dims)).tobytes() == got.tobytes(), f"{label}: two builds differ"
        finally:
            again.close()
        _assert_steps(got, want, label)
        summary = {n: field.summary[n] for n in navmodel.SUMMARY_NAMES}
        assert summary == want_summary, f"{label}: {summary} != {want_summary}"
        assert field.summary["launches"] >= (1 if want_summary["nodes"] else 0)
    except BaseException:
        field.close()
        raise
    return field, want, want_summary


def _assert_steps(got, want, label):
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want.reshape(-1))
        x, y, z = np.unravel_index(bad[0], want.shape)
        raise AssertionError(f"{label}: {len(bad)} positions differ; first ({x}, {y}, {z}): got {got[bad[0]]}, want {want[x, y, z]}")


def _check(ctx, solid, call, goals, label=""):
    field, want, summary = _field(ctx, solid, call, goals, label)
    field.close()
    return want, summary


def _reached_columns(steps):
    """(columns with a reached node, columns with two or more) of a model result."""
    ok = steps["distance"].reshape(-1) >= 0
    cells = np.unique(steps["cell"].reshape(-1, 3)[ok], axis=0)
    _, counts = np.unique(cells[:, [0, 2]], axis=0, return_counts=True)
    return len(counts), int((counts >= 2).sum())


# ---- noise worlds --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", NOISE_DIMS)
@pytest.mark.parametrize("width", [1, 2, 3])
def test_noise_worlds(dims, width):
    """Heights 1, 2, 5 x (stepUp, maxDrop) (0, 0), (1, 3), (h, 4096) over the whole world and an inner box with odd bounds, and 20 random calls."""
    solid, _, ws = nav_noise_world(dims, NOISE_DENSITY[dims, width])
    goals = noise_goals(solid, width)
    want, summary = navmodel.analyse(solid, (0, 0, 0), dims, width, 2, 1, 3, goals)
    columns, several = _reached_columns(want)
    assert columns >= 100 and several >= 20 and summary["nodes"] > summary["reached"] and summary["largestDistance"] >= 2 * TILE, (summary, columns, several)
    assert summary["goalsResolved"] == 2  # the goal inside a solid voxel resolves to nothing, the airborne one to the floor below it
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for height, step_up, max_drop in RULES:
            for name, call in world_calls(dims, width, height, step_up, max_drop).items():
                _check(ctx, solid, call, goals, f"{name}, h {height} s {step_up} m {max_drop}")
        rng = np.random.default_rng(dims[0] * 10 + width + 1000)
        for k in range(20):
            call = random_call(rng, dims)
            _check(ctx, solid, call, goals, f"random call {k} {call}")
    finally:
        ctx.close()
        ws.close()


# ---- the terrain worlds --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((32, 128, 32), True, 3)])
def test_terrain_worlds(dims, sparse, seed):
    """Records with 1 .. 3 runs, run-list columns, both colour layouts; sparse: empty columns, each one node standing on y = 0."""
    rng = np.random.default_rng(seed)
    solid, _, ws = _pick_world(rng, dims, sparse)
    dx, dy, dz = dims
    goals = [(2, dy + 3, 2), (dx - 3, dy - 1, dz - 3), (dx // 2, dy // 2 + 5, dz // 2)]
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for width, height, step_up, max_drop in ((1, 2, 1, 3), (2, 3, 2, 4), (3, 5, 0, 0), (1, 1, 1, 4096)):
            for name, call in world_calls(dims, width, height, step_up, max_drop).items():
                want, summary = _check(ctx, solid, call, goals, f"{name}, w {width} h {height}")
                if name == "whole world" and step_up > 0:
                    assert summary["reached"] > 100, (name, summary)
                if sparse and width == 1 and name == "whole world":
                    assert summary["nodes"] >= int((~solid.any(axis=1)).sum()) > 500
    finally:
        ctx.close()
        ws.close()


# ---- constructed cases on DIMS -----------------------------------------------------------------------------------------------------------------

WHOLE = ((0, 0, 0), DIMS)


def _call(width=1, height=2, step_up=1, max_drop=3, max_steps=0, box=WHOLE):
    return (*box, width, height, step_up, max_drop, max_steps)


def _at(steps, cell):
    return steps[cell[0], cell[1], cell[2]]


def test_a_serpentine_corridor_crosses_the_tiles(built):
    """A corridor one voxel wide, two high under a roof, winding through 64 x 64 columns: 32 rows joined at alternating ends, 2079 cells.  With
    the goal at one end the largest distance is the corridor's length, carried across tile borders hundreds of times."""
    strokes = [_box(FILL, (0, 1, 0), (66, 4, 66), ROCK)]
    for k in range(32):
        strokes.append(_box(CARVE, (1, 1, 2 * k + 1), (65, 3, 2 * k + 2)))
        if k + 1 < 32:
            x = 64 if k % 2 == 0 else 1
            strokes.append(_box(CARVE, (x, 1, 2 * k + 2), (x + 1, 3, 2 * k + 3)))
    ctx, solid, _ = built(strokes)
    cells = 32 * 64 + 31
    want, summary = _check(ctx, solid, _call(1, 2, 0, 0), [(1, 1, 1)], "serpentine")
    assert summary["largestDistance"] == cells - 1 and summary["reached"] == cells and summary["largestDistance"] > 100 * TILE
    assert _at(want, (1, 1, 63))["distance"] == cells - 1  # the far end: row 31 runs back to x = 1


def test_a_bridge_over_a_tunnel_has_two_nodes_with_different_directions(built):
    """A deck at y = 5 over the ground, stairs down at its +X end only; with stepUp 1 and maxDrop 1 the walker on the deck goes +X to the stairs,
    the one in the tunnel beneath it -X straight to the goal."""
    strokes = [_box(FILL, (20, 5, 30), (41, 6, 31), ROCK)] + [_box(FILL, (41 + k, 1, 30), (42 + k, 5 - k, 31), ROCK) for k in range(4)]
    ctx, solid, _ = built(strokes)
    want, _ = _check(ctx, solid, _call(1, 2, 1, 1), [(10, 1, 30)], "bridge")
    below, above = _at(want, (30, 1, 30)), _at(want, (30, 6, 30))
    assert below["cell"].tolist() == [30, 1, 30] and above["cell"].tolist() == [30, 6, 30]
    assert below["direction"] == 0 and below["distance"] == 20 and above["direction"] == 1 and above["distance"] > 40
    assert _at(want, (30, 9, 30))["cell"].tolist() == [30, 6, 30] and _at(want, (30, 3, 30))["cell"].tolist() == [30, 1, 30]  # airborne: the floor below


def test_a_cliff_is_descended_and_not_climbed(built):
    """A plateau 3 high across the whole world, stepUp 1, maxDrop 4: from the top the goal below is a short walk and one drop; with the goal on
    top the ground below is unreached (there is no way round)."""
    ctx, solid, _ = built([_box(FILL, (60, 1, 0), (128, 4, 128), ROCK)])
    want, _ = _check(ctx, solid, _call(1, 2, 1, 4), [(50, 1, 64)], "cliff, goal below")
    assert _at(want, (62, 4, 64))["distance"] == 12 and _at(want, (60, 4, 64))["next"].tolist() == [59, 1, 64]
    want, summary = _check(ctx, solid, _call(1, 2, 1, 4), [(70, 4, 64)], "cliff, goal on top")
    assert _at(want, (59, 1, 64))["cell"].tolist() == [59, 1, 64] and _at(want, (59, 1, 64))["distance"] == -1
    assert summary["reached"] == 68 * 128 and _at(want, (62, 4, 64))["distance"] == 8


def _wall(openings):
    """A wall at x = 40 across the whole world, 10 high, with openings (z0, z1, height) from the ground."""
    return [_box(FILL, (40, 1, 0), (41, 11, 128), ROCK)] + [_box(CARVE, (40, 1, z0), (41, 1 + h, z1)) for z0, z1, h in openings]


def test_a_doorway_too_low_is_closed_and_a_snapshot_stays(built):
    """Height 3: the doorway 2 high at z = 20 is closed, the one 3 high at z = 100 is open, and the walk goes round through it.  Then the low
    doorway is carved to 3: the field built before answers as before (a snapshot), a new build walks straight through."""
    ctx, solid, colour = built(_wall([(20, 21, 2), (100, 101, 3)]))
    call, goals = _call(1, 3, 1, 3), [(30, 1, 20)]
    field, want, _ = _field(ctx, solid, call, goals, "doorways")
    try:
        assert _at(want, (50, 1, 20))["distance"] == 20 + 2 * 80
        assert _at(want, (40, 1, 100))["distance"] > 0 and _at(want, (40, 1, 20))["cell"].tolist() == [-1, -1, -1]  # too low for the body: no cell
        ctx.brush([_box(CARVE, (40, 3, 20), (41, 4, 21))], 5)
        solid[40, 3, 20] = False
        _assert_steps(field.query(_positions(DIMS)), want, "the snapshot after the carve")
    finally:
        field.close()
    want, _ = _check(ctx, solid, call, goals, "after the carve")
    assert _at(want, (50, 1, 20))["distance"] == 20 and _at(want, (40, 1, 20))["distance"] == 10


def test_a_gap_narrower_than_the_body_is_closed(built):
    """Openings 2 and 3 wide in the wall: width 3 goes round through the wide one, width 2 straight through the narrow one."""
    ctx, solid, _ = built(_wall([(20, 22, 10), (100, 103, 10)]))
    want, _ = _check(ctx, solid, _call(3, 3, 1, 3), [(30, 1, 20)], "width 3")
    assert _at(want, (50, 1, 20))["distance"] == 20 + 2 * 80 and _at(want, (39, 1, 20))["cell"].tolist() == [-1, -1, -1]
    want, _ = _check(ctx, solid, _call(2, 3, 1, 3), [(30, 1, 20)], "width 2")
    assert _at(want, (50, 1, 20))["distance"] == 20


def test_a_riser_must_be_clear_in_the_source(built):
    """Height 3, stepUp 1 onto a block one high: the source needs clear air up to y' + h = 5.  Under a ceiling voxel at y = 4 the source is clear
    only up to y' + h - 1 -- it is still a stand cell, but the step does not exist (nor the one down into it): the way leads round.  The same
    block without the ceiling is one step away."""
    strokes = [_box(FILL, (31, 1, 30), (32, 2, 31), ROCK), _box(FILL, (30, 4, 30), (31, 5, 31), ROCK),
               _box(FILL, (31, 1, 90), (32, 2, 91), ROCK)]
    ctx, solid, _ = built(strokes)
    want, _ = _check(ctx, solid, _call(1, 3, 1, 3), [(31, 2, 30), (31, 2, 90)], "riser")
    assert _at(want, (30, 1, 30))["cell"].tolist() == [30, 1, 30] and _at(want, (30, 1, 30))["distance"] == 3
    assert _at(want, (30, 1, 90))["distance"] == 1 and _at(want, (30, 1, 90))["next"].tolist() == [31, 2, 90]


def test_goals_on_the_edge_and_on_the_floor_and_max_steps(built):
    """A hole in the floor of the corner column (0, 0): its cell stands on y = 0.  maxSteps = the distance of a chosen cell: that cell is
    reached, its farther neighbour is not."""
    ctx, solid, _ = built([_box(CARVE, (0, 0, 0), (1, 1, 1))])
    want, summary = _check(ctx, solid, _call(1, 2, 1, 3), [(0, 0, 0), (127, 40, 127)], "edge goals")
    assert _at(want, (0, 0, 0))["cell"].tolist() == [0, 0, 0] and _at(want, (0, 0, 0))["distance"] == 0 and summary["goalsResolved"] == 2
    assert _at(want, (1, 1, 0))["next"].tolist() == [0, 0, 0] and _at(want, (1, 1, 0))["direction"] == 0
    assert _at(want, (127, 1, 127))["distance"] == 0 and _at(want, (127, 1, 126))["direction"] == 5
    want, summary = _check(ctx, solid, _call(1, 2, 1, 3, max_steps=10), [(64, 1, 64)], "maxSteps")
    assert _at(want, (74, 1, 64))["distance"] == 10 and _at(want, (75, 1, 64))["distance"] == -1 and _at(want, (75, 1, 64))["cell"].tolist() == [75, 1, 64]
    assert summary["largestDistance"] == 10 and summary["reached"] == 2 * 10 * 11 + 1


def test_columns_of_many_nodes_take_the_global_memory_path(built):
    """Alternating one-voxel slabs up the full height, height 1: 32 nodes per column.  One such column alone, and a block of 24 x 24 of them:
    every tile that holds 256 of its columns has 8192 nodes and more, far beyond the 1536 the tile path keeps in LDS, so those tiles relax in
    global memory -- and give the model's bytes."""
    slabs = range(2, DIMS[1], 2)
    strokes = [_box(FILL, (80, y, 80), (104, y + 1, 104), ROCK) for y in slabs] + [_box(FILL, (10, y, 10), (11, y + 1, 11), ROCK) for y in slabs]
    ctx, solid, _ = built(strokes)
    want, summary = _check(ctx, solid, _call(1, 1, 1, 4096), [(5, 1, 5)], "slabs")
    per_column = len({int(c) for c in want["cell"][90, :, 90][:, 1]} - {-1})
    assert per_column == 32 and per_column * TILE * TILE > TILE_NODES
    assert summary["reached"] == summary["nodes"] and _at(want, (90, 63, 90))["distance"] > 0


# ---- re-goal, device query, the walk, errors -----------------------------------------------------------------------------------------------------

@pytest.fixture()
def noise():
    """The (32, 32, 32) noise world of width 2 on the device -> (ctx, solid, goals)."""
    dims = NOISE_DIMS[0]
    solid, _, ws = nav_noise_world(dims, NOISE_DENSITY[dims, 2])
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    yield ctx, solid, noise_goals(solid, 2)
    ctx.close()
    ws.close()


def test_new_goals_equal_a_fresh_build(noise):
    ctx, solid, goals = noise
    dims = tuple(solid.shape)
    call = ((0, 0, 0), dims, 2, 3, 2, 4, 0)
    cells = navmodel.stand_cells(solid, 2, 5)
    other = [tuple(int(v) for v in cells[0]), tuple(int(v) for v in cells[-1])]
    field, want, want_summary = _field(ctx, solid, call, goals, "the first goals")
    try:
        first = field.query(_positions(dims))
        want_b, summary_b = navmodel.analyse(solid, *call[:6], other, 7)
        got_summary = field.goals(other, max_steps=7)
        _assert_steps(field.query(_positions(dims)), want_b, "new goals")
        assert {n: got_summary[n] for n in navmodel.SUMMARY_NAMES} == summary_b and summary_b["largestDistance"] == 7
        fresh = ctx.nav_build(call[0], call[1], other, width=2, height=3, step_up=2, max_drop=4, max_steps=7)
        assert fresh.query(_positions(dims)).tobytes() == field.query(_positions(dims)).tobytes()
        fresh.close()
        back = field.goals(goals)
        assert field.query(_positions(dims)).tobytes() == first.tobytes() and {n: back[n] for n in navmodel.SUMMARY_NAMES} == want_summary
    finally:
        field.close()


def test_device_query_on_a_callers_stream(noise):
    import torch

    ctx, solid, goals = noise
    dims = tuple(solid.shape)
    field, want, _ = _field(ctx, solid, ((0, 0, 0), dims, 2, 3, 2, 4, 0), goals, "device query")
    try:
        rng = np.random.default_rng(5)
        cells = rng.integers(-3, 36, size=(4096, 3)).astype(np.int32)
        cells[:5] = [[-1, 5, 5], [5, -1, 5], [40, 5, 5], [5, 5, -2**31], [5, 2**31 - 1, 5]]
        cells[1::97] = [2**31 - 1, 2**31 - 1, 2**31 - 1]
        cells[2::97] = [-2**31, -2**31, -2**31]
        host_steps = field.query(cells)
        assert host_steps.tobytes() == navmodel.query(want, cells).tobytes()
        outside = (cells[:, 0] < 0) | (cells[:, 0] >= dims[0]) | (cells[:, 2] < 0) | (cells[:, 2] >= dims[2]) | (cells[:, 1] < 0)
        assert outside.sum() > 500 and (host_steps["cell"][outside] == -1).all() and (host_steps["distance"][outside] == -1).all()
        assert (host_steps["cell"][:, 0] >= 0).sum() > 500
        stream = torch.cuda.Stream()
        d_cells = torch.from_numpy(cells).cuda()
        d_steps = torch.full((len(cells) + 2, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # one guard record on either side
        torch.cuda.synchronize()
        field.query_device(len(cells), d_cells.data_ptr(), d_steps[1:].data_ptr(), stream.cuda_stream)
        stream.synchronize()
        out = d_steps.cpu().numpy()
        assert out[1:-1].tobytes() == host_steps.tobytes()
        assert (out[0] == 0x5A5A5A5A).all() and (out[-1] == 0x5A5A5A5A).all(), "the query wrote outside its steps"
    finally:
        field.close()


def test_the_walk_follows_next_with_world_move(noise):
    """From 64 reached cells (width 2, height 3, stepUp 2, maxDrop 4): per step one cvx_world_move sideways with stepUp = the rise and one down by
    maxDrop.  The body ends exactly on `next` every time, never starts in solid, and reaches a goal in exactly `distance` steps."""
    ctx, solid, goals = noise
    dims = tuple(solid.shape)
    field, want, summary = _field(ctx, solid, ((0, 0, 0), dims, 2, 3, 2, 4, 0), goals, "walk")
    try:
        got = field.query(_positions(dims)).reshape(dims)
        starts = walk_starts(want, 64, 11)
        longest = max(int(want[x, y, z]["distance"]) for x, y, z in starts)
        assert walk(ctx.world_move, got, starts, 2, 3, 4) == longest >= 10
    finally:
        field.close()


def test_errors(noise):
    ctx, solid, goals = noise
    L = gpu.lib()
    dims = tuple(solid.shape)
    g = np.array(goals, dtype=np.int32)

    def build(box_min=(0, 0, 0), box_max=dims, width=2, height=3, step_up=1, max_drop=3, max_steps=0, goals_ptr=g.ctypes.data, count=3, params=True, out=True):
        p = gpu.NavParams((C.c_int32 * 3)(*box_min), (C.c_int32 * 3)(*box_max), width, height, step_up, max_drop, max_steps, 0)
        handle = C.c_void_p(1)
        rc = L.cvx_world_nav_build(ctx._h, C.byref(p) if params else None, goals_ptr, count, C.byref(handle) if out else None, None, None)
        assert rc == 0 or not out or not handle.value, "a failing build left a field"
        if rc == 0:
            L.cvx_nav_field_destroy(handle)
        return rc

    assert build() == 0
    bad = [build(params=False), build(goals_ptr=None), build(out=False), build(box_min=(5, 0, 0), box_max=(5, 32, 32)), build(box_min=(0, 9, 0), box_max=(32, 3, 32)),
           build(box_min=(40, 0, 0), box_max=(50, 32, 32)), build(box_min=(0, -9, 0), box_max=(32, 0, 32)), build(width=0), build(width=9), build(height=0),
           build(height=65), build(step_up=-1), build(step_up=4), build(max_drop=-1), build(max_drop=4097), build(max_steps=-1), build(count=0), build(count=-1),
           build(count=4097)]
    assert bad == [-1] * len(bad), bad
    assert build(box_min=(0, 0, 0), box_max=(1, 32, 32)) == 0  # narrower than the body: CVX_OK and an empty field
    empty = ctx.nav_build((0, 0, 0), (1, 32, 32), goals, width=2, height=3)
    assert empty.summary["nodes"] == 0 and (empty.query(_positions(dims)[:1000])["cell"] == -1).all()
    empty.close()
    field = ctx.nav_build((0, 0, 0), dims, goals, width=2, height=3)
    other = gpu.Context(0)
    try:
        steps = np.zeros(4, dtype=gpu.NAV_STEP_DTYPE)
        cells = np.zeros((4, 3), dtype=np.int32)
        q = lambda c, f, n, cp, sp: L.cvx_nav_query(c, f, n, cp, sp)  # noqa: E731
        qd = lambda c, f, n, cp, sp: L.cvx_nav_query_device(c, f, n, cp, sp, None)  # noqa: E731
        for call in (q, qd):
            assert call(ctx._h, field._h, -1, cells.ctypes.data, steps.ctypes.data) == -1
            assert call(ctx._h, None, 4, cells.ctypes.data, steps.ctypes.data) == -1
            assert call(ctx._h, field._h, 4, None, steps.ctypes.data) == -1
            assert call(ctx._h, field._h, 4, cells.ctypes.data, None) == -1
            assert call(other._h, field._h, 4, cells.ctypes.data, steps.ctypes.data) == -1  # a field of another context
            assert call(None, field._h, 4, cells.ctypes.data, steps.ctypes.data) == -1
        assert L.cvx_nav_query(ctx._h, field._h, 0, cells.ctypes.data, steps.ctypes.data) == 0
        goals_call = lambda c, f, ptr, n, ms: L.cvx_nav_field_goals(c, f, ptr, n, ms, None, None)  # noqa: E731
        assert goals_call(other._h, field._h, g.ctypes.data, 3, 0) == -1
        assert goals_call(ctx._h, None, g.ctypes.data, 3, 0) == -1
        assert goals_call(ctx._h, field._h, None, 3, 0) == -1
        assert goals_call(ctx._h, field._h, g.ctypes.data, 0, 0) == -1
        assert goals_call(ctx._h, field._h, g.ctypes.data, 4097, 0) == -1
        assert goals_call(ctx._h, field._h, g.ctypes.data, 3, -1) == -1
        assert goals_call(ctx._h, field._h, g.ctypes.data, 3, 0) == 0
        p = gpu.NavParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8), 1, 2, 1, 3, 0, 0)
        handle = C.c_void_p(1)
        assert L.cvx_world_nav_build(other._h, C.byref(p), g.ctypes.data, 3, C.byref(handle), None, None) == -3 and not handle.value  # CVX_ERR_NOT_READY
        L.cvx_nav_field_destroy(None)
    finally:
        other.close()
        field.close()
    # the context closes the fields it still owns
    left = ctx.nav_build((0, 0, 0), dims, goals, width=2, height=3)
    assert left in ctx._nav_fields
