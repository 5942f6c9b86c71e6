"""CPU (no GPU needed): the rules behind cvx_world_nav_build / cvx_nav_query (cpuvox_amd/csrc/cvx_nav.h), compiled for the host through
tests/nav_rules.cpp (which drives them sequentially: node lists, Bellman-Ford to the fixpoint, next, query), against the independent dense model
of tests/navmodel.py (blocked voxels by OR-ed shifts, clear ranges by cumulative sums, scipy's Dijkstra; it knows no intervals).

- World mode: the noise worlds and the terrain worlds of _pick_world uploaded into a host-only context; for the whole world, an inner box with
  odd bounds and random calls, over widths 1 .. 3, heights 1, 2, 5 and (stepUp, maxDrop) in (0, 0), (1, 3), (h, 4096), the cvx_nav_step of EVERY
  voxel position of the world and the deterministic summary fields equal the model's exactly.  Widths 8, 7 and 5 with heights 64, 63 and 1 (the
  largest the rule allows) on the constructed wall of limitworlds.nav_wide_world.
- Every argument error that needs no device (the header's mirrors: tests/test_abi_mirrors.py).

The noise worlds: noise_world's 70 % solid leaves little standing room for a body wider than a voxel, so width w draws the same generator at
NOISE_DENSITY[dims, w] (nav_noise_world).  The densities were chosen with the model alone so that the preconditions of the GPU test hold
(tests/test_gpu_world_nav.py lists the model's counts)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import limitworlds as LW
import movemodel
import navmodel
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE_DIMS = [(32, 32, 32), (16, 64, 32)]
NOISE_DENSITY = {((32, 32, 32), 1): 0.3, ((32, 32, 32), 2): 0.08, ((32, 32, 32), 3): 0.03, ((16, 64, 32), 1): 0.25, ((16, 64, 32), 2): 0.1, ((16, 64, 32), 3): 0.05}
RULES = [(h, s, m) for h in (1, 2, 5) for s, m in ((0, 0), (1, 3), (h, 4096))]


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("nav_rules", tmp_path_factory.mktemp("nav"))


def nav_noise_world(dims, density):
    """noise_world's generator (np.random.default_rng(1).random(dims)) at another density -> (solid, colour, ws)."""
    solid = np.random.default_rng(1).random(dims) < density
    x, y, z = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[x, y, z] = (0xFF000000 | ((x * 2654435761 + y * 40503 + z * 2246822519) >> 7) & 0xFFFFFF).astype(np.uint32)
    ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=2)
    return solid, colour, ws


def noise_goals(solid, width):
    """Three goals: one inside a solid voxel (it resolves to nothing), one airborne (two voxels above a floor: it resolves downward) and one on
    the floor it names.  The solid one is the first solid voxel in (x, y, z) order; the other two come from the stand cells of a body 5 high (so
    that they resolve for every height of the tests): the one nearest to the world's centre and, for the airborne goal, the one nearest to the
    point a quarter into the world (L1 distance, the first such cell in (x, y, z) order)."""
    dx, dy, dz = solid.shape
    cells = navmodel.stand_cells(solid, width, 5)

    def nearest(p):
        return [int(v) for v in cells[np.argmin(np.abs(cells - np.array(p)).sum(axis=1))]]

    a, b = nearest((dx // 2, dy // 2, dz // 2)), nearest((dx // 4, dy // 2, dz // 4))
    return [tuple(int(v) for v in np.argwhere(solid)[0]), (b[0], b[1] + 2, b[2]), tuple(a)]


def random_call(rng, dims):
    """(box_min, box_max, width, height, step_up, max_drop, max_steps): a random box partly outside the world (the whole world when nothing of it
    is inside) and a random rule."""
    box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
    box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
    if navmodel.clip_box(dims, box_min, box_max) is None:
        box_min, box_max = [0, 0, 0], list(dims)
    h = int(rng.choice([1, 2, 5]))
    s, m = [(0, 0), (1, 3), (h, 4096)][int(rng.integers(0, 3))]
    return box_min, box_max, int(rng.integers(1, 4)), h, min(s, h), m, int(rng.choice([0, 0, 3, 12]))


def run_world(rules, tmp_path, ws, box_min, box_max, width, height, step_up, max_drop, max_steps, goals):
    """tests/nav_rules.cpp `world` on LOD 0 of ws -> (steps[x, y, z], summary dict, nodes, ms)."""
    info = ws.info(0)
    blob, goals_in, out = tmp_path / "world.bin", tmp_path / "goals.bin", tmp_path / "steps.bin"
    if not blob.exists():
        blob.write_bytes(ws.storage(0).tobytes())
    goals_in.write_bytes(np.asarray(goals, dtype=np.int32).reshape(-1, 3).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                    *[str(int(v)) for v in box_min], *[str(int(v)) for v in box_max], str(width), str(height), str(step_up), str(max_drop),
                                    str(max_steps), str(goals_in), str(out)], text=True)
    m = re.match(r"nodes (\d+) ms ([0-9.]+)", text)
    assert m, text
    raw = out.read_bytes()
    summary = np.frombuffer(raw[:40], dtype=gpu.NAV_SUMMARY_DTYPE)[0]
    steps = np.frombuffer(raw[40:], dtype=gpu.NAV_STEP_DTYPE).reshape(info.dimX, info.dimY, info.dimZ)
    return steps, {n: int(summary[n]) for n in navmodel.SUMMARY_NAMES}, int(m.group(1)), float(m.group(2))


def assert_field(got, summary, solid, call, goals, label):
    """The steps of every voxel position and the summary against the model."""
    box_min, box_max, width, height, step_up, max_drop, max_steps = call
    want, want_summary = navmodel.analyse(solid, box_min, box_max, width, height, step_up, max_drop, goals, max_steps)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        x, y, z = bad[0]
        raise AssertionError(f"{label}: {len(bad)} positions differ; first ({x}, {y}, {z}): got {got[x, y, z]}, want {want[x, y, z]}")
    return want_summary


def world_calls(dims, width, height, step_up, max_drop):
    dx, dy, dz = dims
    return {
        "whole world": ((0, 0, 0), dims, width, height, step_up, max_drop, 0),
        "inner box with odd bounds": ((3, 1, 5), (dx - 4, dy - 3, dz - 1), width, height, step_up, max_drop, 0),
    }


@pytest.mark.parametrize("dims", NOISE_DIMS)
@pytest.mark.parametrize("width", [1, 2, 3])
def test_noise_worlds_equal_the_model(rules, tmp_path, dims, width):
    solid, _, ws = nav_noise_world(dims, NOISE_DENSITY[dims, width])
    try:
        goals = noise_goals(solid, width)
        reached = 0
        for height, step_up, max_drop in RULES:
            for name, call in world_calls(dims, width, height, step_up, max_drop).items():
                got, summary, _, _ = run_world(rules, tmp_path, ws, *call, goals)
                want = assert_field(got, summary, solid, call, goals, f"{name}, h {height} s {step_up} m {max_drop}")
                if name == "whole world":
                    assert want["goalsResolved"] == 2, want
                reached += want["reached"]
        assert reached > 1000
        rng = np.random.default_rng(dims[0] * 10 + width)
        for k in range(20):
            call = random_call(rng, dims)
            got, summary, _, _ = run_world(rules, tmp_path, ws, *call, goals)
            assert_field(got, summary, solid, call, goals, f"random call {k} {call}")
    finally:
        ws.close()


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((32, 128, 32), True, 3)])
def test_terrain_worlds_equal_the_model(rules, tmp_path, dims, sparse, seed):
    """Records with 1 .. 3 runs, run-list columns, both colour layouts, empty columns (one node standing on y = 0)."""
    rng = np.random.default_rng(seed)
    solid, _, ws = _pick_world(rng, dims, sparse)
    try:
        dx, dy, dz = dims
        goals = [(2, dy + 3, 2), (dx - 3, dy - 1, dz - 3), (dx // 2, dy // 2 + 5, dz // 2)]
        empty = int((~solid.any(axis=1)).sum())
        assert (empty > 500) == sparse
        for width, height, step_up, max_drop in ((1, 2, 1, 3), (2, 3, 2, 4), (3, 5, 0, 0), (1, 1, 1, 4096)):
            for name, call in world_calls(dims, width, height, step_up, max_drop).items():
                got, summary, _, _ = run_world(rules, tmp_path, ws, *call, goals)
                want = assert_field(got, summary, solid, call, goals, f"{name}, w {width} h {height}")
                if name == "whole world" and step_up > 0:
                    assert want["reached"] > 100 and want["goalsResolved"] >= 2, (name, want)
                if sparse and width == 1 and name == "whole world":
                    assert want["nodes"] >= empty  # an empty column is one node on y = 0
    finally:
        ws.close()


def wide_world():
    """limitworlds.nav_wide_world as (solid, ws)."""
    solid = LW.nav_wide_world()
    x, y, z = np.nonzero(solid)
    ws = host.WorldSet.from_voxels(LW.NAV_WIDE_DIMS, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF808080, dtype=np.uint32), threads=2)
    return solid, ws


def test_the_widest_and_tallest_body_equals_the_model(rules, tmp_path):
    """Widths 8 (kNavMaxWidth), 7 and 5 with heights 64 (kNavMaxHeight), 63 and 1: the w x w union walk of NavNextInterval at its largest, on a
    wall whose openings are exactly 8 and 7 wide and leave exactly 64 and 63 clear, with two steps behind it."""
    solid, ws = wide_world()
    try:
        assert [LW.nav_wide_passable(w, h) for w, h, _, _ in LW.NAV_WIDE_RULES] == [[0], [0, 2], [0, 1], [0, 1], [0, 1, 2]]
        near = {}
        for width, height, step_up, max_drop in LW.NAV_WIDE_RULES:
            for name, call in world_calls(LW.NAV_WIDE_DIMS, width, height, step_up, max_drop).items():
                got, summary, _, _ = run_world(rules, tmp_path, ws, *call, [LW.NAV_WIDE_GOAL])
                assert_field(got, summary, solid, call, [LW.NAV_WIDE_GOAL], f"{name}, w {width} h {height}")
                if name == "whole world":
                    LW.assert_wide_openings(got, width, height)
                    near[width, height] = int(got[10, 1, 23]["distance"])
        assert near[8, 63] < near[8, 64] and near[8, 63] > 0, "one voxel less of height opens the nearer doorway"
        assert near[5, 1] == -1, "no step up: the goal on the steps is out of reach"
    finally:
        ws.close()


# ---- the walk: next against the move rule ---------------------------------------------------------------------------------------------------------

def walk(move, steps, starts, width, height, max_drop):
    """Follows `next` from every start with two moves per step (`move`: bodies -> MOVE_RESULT_DTYPE array; cvx_world_move on the GPU, tests/movemodel.py here): -> steps made."""
    unit = gpu.MOVE_UNIT
    at = np.array(starts, dtype=np.int64)
    left = np.array([int(steps[x, y, z]["distance"]) for x, y, z in at])
    made = 0
    while (left > 0).any():
        live = np.flatnonzero(left > 0)
        here = np.array([steps[x, y, z] for x, y, z in at[live]])
        assert (here["cell"] == at[live]).all() and (here["distance"] == left[live]).all()
        nxt = here["next"].astype(np.int64)
        bodies = [{"pos": (at[i] * unit).tolist(), "size": [width * unit, height * unit, width * unit],
                   "delta": [int(n[0] - at[i][0]) * unit, 0, int(n[2] - at[i][2]) * unit], "stepUp": max(0, int(n[1] - at[i][1])) * unit,
                   "flags": gpu.MOVE_SOLID_BELOW} for i, n in zip(live, nxt)]
        first = move(bodies)
        assert not (first["flags"] & gpu.MOVED_STARTS_SOLID).any()
        second = move([{"pos": r["pos"].tolist(), "size": b["size"], "delta": [0, -max_drop * unit, 0], "stepUp": 0, "flags": gpu.MOVE_SOLID_BELOW}
                       for r, b in zip(first, bodies)])
        assert not (second["flags"] & gpu.MOVED_STARTS_SOLID).any() and (second["flags"] & gpu.MOVED_RESTING).all()
        assert (second["pos"] == nxt * unit).all(), f"step {made}: the body ends at {second['pos'].tolist()}, next is {nxt.tolist()}"
        at[live] = nxt
        left[live] -= 1
        made += 1
    assert all(int(steps[x, y, z]["distance"]) == 0 for x, y, z in at)
    return made


def walk_starts(steps, count, seed):
    reached = np.argwhere(steps["distance"] > 0)
    cells = np.unique(steps["cell"][reached[:, 0], reached[:, 1], reached[:, 2]], axis=0)
    return cells[np.random.default_rng(seed).choice(len(cells), size=count, replace=False)]


def test_the_walk_follows_next_on_the_models():
    """The field's rule against cvx_world_move's, both as dense models (tests/navmodel.py, tests/movemodel.py): from 16 reached cells of the
    width-2 noise world (height 3, stepUp 2, maxDrop 4) the body ends exactly on `next` after every step and reaches a goal in `distance` steps.
    The GPU test makes the same walk with the two device calls."""
    dims = NOISE_DIMS[0]
    solid = np.random.default_rng(1).random(dims) < NOISE_DENSITY[dims, 2]
    steps, summary = navmodel.analyse(solid, (0, 0, 0), dims, 2, 3, 2, 4, noise_goals(solid, 2))
    assert summary["reached"] > 500

    def move(bodies):
        out = np.zeros(len(bodies), dtype=gpu.MOVE_RESULT_DTYPE)
        for i, b in enumerate(bodies):
            pos, flags = movemodel.move(solid, b)
            out[i] = (pos, flags)
        return out

    starts = walk_starts(steps, 16, 11)
    assert walk(move, steps, starts, 2, 3, 4) == max(int(steps[x, y, z]["distance"]) for x, y, z in starts)


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_nav_calls_fail_cleanly_without_a_context_or_world(rules):
    # a context without a device or world (tests/nav_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY; no failing build leaves a field
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 23 + [-3, 0], codes
    L = gpu.lib()
    L.cvx_nav_field_destroy(None)
    p = gpu.NavParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8), 1, 2, 1, 3, 0, 0)
    goals = (C.c_int32 * 3)(1, 1, 1)
    field = C.c_void_p(1)
    assert L.cvx_world_nav_build(None, C.byref(p), goals, 1, C.byref(field), None, None) == -1 and not field.value
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_nav_build(h, C.byref(p), goals, 1, C.byref(field), None, None) == -3 and not field.value
        finally:
            L.cvx_destroy(h)
