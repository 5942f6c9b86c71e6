"""CPU (no GPU needed): the rule behind cvx_world_move (cpuvox_amd/csrc/cvx_move.h), compiled for the host through tests/move_rules.cpp, against
the independent dense model of tests/movemodel.py.  The rule is integer from end to end, so every comparison is exact and nothing is exempt.

- Cases mode: 2000 random small worlds (seed 2033) of up to 4 x 4 random columns (records with 1..3 runs and listed columns, foreign encodings
  with split runs and shared colours) with 16 bodies each: starts partly outside the world and embedded, sizes from one unit to several voxels
  (a few up to the maximum), deltas from 0 to the maximum, every flag combination, stepUp 0 and positive, repeat on and off.  The invariant
  (a body that does not start in solid never ends in solid) is checked on every one of them with the model's overlap test.
- World mode: the worlds of the pick test uploaded into a host-only context (both colour layouts, run-list columns), 3000 bodies each.
- Hand-derived cases whose results are asserted as literals.
- Every INVALID_ARGUMENT and NOT_READY case (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import movemodel
import pyworld
import ruleslib
from cpuvox_amd import gpu
from movemodel import RESTING, STARTS_SOLID, STEPPED, UNIT
from test_world_brush_cpu import _pick_world, _random_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = UNIT
MINUS_X, PLUS_X, MINUS_Y, PLUS_Y, MINUS_Z, PLUS_Z = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("move_rules", tmp_path_factory.mktemp("move"), "-O2")  # (the GPU test and tools/move_bench.py build it so too)


# ---- random bodies ---------------------------------------------------------------------------------------------------------------------------------

def random_body(rng, dims, big=0.03):
    """One random body around a world of `dims` voxels (the GPU test uses it too)."""
    size = []
    for _ in range(3):
        kind = rng.random()
        if kind < 0.1:
            s = 1
        elif kind < 0.45:
            s = int(rng.integers(1, U + 1))
        elif kind < 1.0 - big:
            s = int(rng.integers(1, 3 * U + 1))
        else:
            s = int(rng.choice([64 * U, int(rng.integers(3 * U, 64 * U + 1))]))
        size.append(s)
    pos = []
    for a in range(3):
        p = int(rng.integers(-2 * U - size[a], (dims[a] + 2) * U))
        if rng.random() < 0.3:
            p = (p // U) * U  # on the voxel grid: flush contacts and resting bodies
        pos.append(p)
    delta = []
    for _ in range(3):
        kind = rng.random()
        if kind < 0.25:
            d = 0
        elif kind < 0.55:
            d = int(rng.integers(-U, U + 1))
        elif kind < 0.85:
            d = int(rng.integers(-8 * U, 8 * U + 1))
        elif kind < 0.93:
            d = int(rng.integers(-8, 9)) * U
        else:
            d = int(rng.choice([-1, 1])) * int(rng.choice([movemodel.MAX_DELTA, int(rng.integers(8 * U, movemodel.MAX_DELTA + 1))]))
        delta.append(d)
    step_up = int(rng.choice([0, 0, 1, 255, 256, 300, 4 * U, int(rng.integers(1, 4 * U + 1))]))
    return movemodel.body(pos, size, delta, step_up, int(rng.integers(0, 4)))


def random_bodies(rng, solid, repeat, n, settled=0.35):
    """n random bodies; a fraction of them starts where the model says an earlier fall or push ended (resting on the ground, flush against a
    wall), with a new delta."""
    out = []
    for _ in range(n):
        b = random_body(rng, solid.shape)
        if rng.random() < settled:
            first = dict(b, delta=[int(rng.integers(-2 * U, 2 * U + 1)), -int(rng.integers(1, movemodel.MAX_DELTA + 1)), int(rng.integers(-2 * U, 2 * U + 1))])
            pos, _ = movemodel.move(solid, first, repeat)
            if all(abs(p) <= movemodel.MAX_POS for p in pos):
                b = dict(b, pos=pos)
        out.append(b)
    return out


def body_words(b):
    return [*b["pos"], *b["size"], *b["delta"], b["stepUp"], b["flags"], 0]


def bodies_to_array(bodies):
    return np.array([body_words(b) for b in bodies], dtype=np.int32).view(gpu.MOVE_BODY_DTYPE).reshape(-1)


def model_results(solid, bodies, repeat):
    out = np.zeros(len(bodies), dtype=gpu.MOVE_RESULT_DTYPE)
    for i, b in enumerate(bodies):
        pos, flags = movemodel.move(solid, b, repeat)
        out[i]["pos"], out[i]["flags"] = pos, flags
    return out


# ---- cases mode ----------------------------------------------------------------------------------------------------------------------------------------

def _run_cases(rules, tmp_path, cases):
    """cases: (dim_y, gx, gz, stride, columns [(base, runs, colours)], repeat, bodies) -> a MOVE_RESULT_DTYPE array per case"""
    words = []
    for dim_y, gx, gz, stride, columns, repeat, bodies in cases:
        words += ruleslib.world_words(dim_y, gx, gz, stride, columns) + [int(repeat), len(bodies)]
        for b in bodies:
            words += body_words(b)
    out = ruleslib.run_cases(rules, "cases", tmp_path, words, dtype=gpu.MOVE_RESULT_DTYPE)
    assert len(out) == sum(len(c[6]) for c in cases)
    results, at = [], 0
    for c in cases:
        results.append(out[at:at + len(c[6])])
        at += len(c[6])
    return results


def test_rules_match_the_dense_model_on_random_small_worlds(rules, tmp_path):
    rng = np.random.default_rng(2033)
    cases, solids, models = [], [], []
    split = listed_like = 0
    for _ in range(2000):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        gx, gz = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        stride = int(rng.choice([1, 32]))
        solid = np.zeros((gx, dim_y, gz), dtype=bool)
        columns = []
        for k in range(gx * gz):
            runs, colours, _, _ = _random_column(rng, dim_y)
            x, z = k // gz, k % gz
            top = dim_y
            previous_solid = False
            for ci, n in runs:
                if ci >= 0:
                    solid[x, top - n:top, z] = True
                    split += previous_solid
                previous_solid = ci >= 0
                top -= n
            listed_like += len([ci for ci, _ in runs if ci >= 0]) > 3
            columns.append((32 + k * 20000 + int(rng.integers(0, 100)), runs, colours))
        repeat = bool(rng.integers(0, 2))
        bodies = random_bodies(rng, solid, repeat, 16)
        cases.append((dim_y, gx, gz, stride, columns, repeat, bodies))
        solids.append(solid)
        models.append(model_results(solid, bodies, repeat))
    results = _run_cases(rules, tmp_path, cases)
    bad = [(i, k) for i in range(len(cases)) for k in range(16) if results[i][k] != models[i][k]]
    if bad:
        i, k = bad[0]
        raise AssertionError(f"{len(bad)} of {16 * len(cases)} bodies differ; first: case {i} body {k} {cases[i][6][k]} repeat {cases[i][5]}\n"
                             f" got {results[i][k]}\nwant {models[i][k]}\nworld {solids[i].shape}: {cases[i][4]}")
    # the invariant, and what the cases cover
    seen = dict(stepped=0, resting=0, starts_solid=0, left_solid=0, repeat=0, free=0, outside=0, big=0, full_delta=0)
    blocked = np.zeros(6, dtype=np.int64)
    flag_sets = set()
    for (dim_y, gx, gz, _, _, repeat, bodies), solid, got in zip(cases, solids, results):
        for b, r in zip(bodies, got):
            flags, pos = int(r["flags"]), [int(v) for v in r["pos"]]
            ends_solid = movemodel.overlaps(solid, pos, b["size"], b["flags"], repeat)
            if not flags & STARTS_SOLID:
                assert not ends_solid, f"{b} (repeat {repeat}) ends inside a solid voxel at {pos}"
            seen["stepped"] += bool(flags & STEPPED)
            seen["resting"] += bool(flags & RESTING)
            seen["starts_solid"] += bool(flags & STARTS_SOLID)
            seen["left_solid"] += bool(flags & STARTS_SOLID) and not ends_solid
            seen["repeat"] += repeat
            seen["free"] += flags == 0 and any(b["delta"])
            seen["outside"] += any(b["pos"][a] < 0 or b["pos"][a] + b["size"][a] > U * solid.shape[a] for a in range(3))
            seen["big"] += max(b["size"]) > 3 * U
            seen["full_delta"] += max(abs(d) for d in b["delta"]) == movemodel.MAX_DELTA
            blocked += [(flags >> k) & 1 for k in range(6)]
            flag_sets.add((b["flags"], b["stepUp"] > 0))
    assert len(flag_sets) == 8 and split > 100 and listed_like > 300, (flag_sets, split, listed_like)
    assert seen["stepped"] >= 50 and seen["resting"] > 1000 and seen["starts_solid"] > 1000 and seen["left_solid"] > 200 and seen["free"] > 1000, seen
    assert seen["repeat"] > 10000 and seen["outside"] > 3000 and seen["big"] > 500 and seen["full_delta"] > 500 and (blocked > 500).all(), (seen, blocked)


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------------

def run_world(rules, tmp_path, blob, dims, column_count, repeat, bodies):
    """tests/move_rules.cpp `world` on an LOD-0 blob -> (MOVE_RESULT_DTYPE array, colorShift, listed columns, ms); bodies: a MOVE_BODY_DTYPE array"""
    world, src, dst = tmp_path / "world.bin", tmp_path / "bodies.bin", tmp_path / "results.bin"
    world.write_bytes(blob)
    src.write_bytes(bodies.tobytes())
    text = subprocess.check_output([rules, "world", str(world), *[str(d) for d in dims], str(column_count), str(int(repeat)), str(src), str(dst)], text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) bodies (\d+) ms ([0-9.]+)", text)
    assert m and int(m.group(3)) == len(bodies), text
    return np.frombuffer(dst.read_bytes(), dtype=gpu.MOVE_RESULT_DTYPE), int(m.group(1)), int(m.group(2)), float(m.group(4))


WORLDS = [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((64, 256, 64), True, 3)]


def world_bodies(seed, solid, repeat, n):
    """The bodies of the world tests (the GPU test runs the same ones): seed = the world's + 200 (+ 1 repeating)."""
    return random_bodies(np.random.default_rng(seed + 200 + int(repeat)), solid, repeat, n)


@pytest.mark.parametrize("dims,sparse,seed", WORLDS)
def test_uploaded_worlds_match_the_dense_model(rules, tmp_path, dims, sparse, seed):
    solid, _, ws = _pick_world(np.random.default_rng(seed), dims, sparse)
    try:
        info = ws.info(0)
        blob = ws.storage(0).tobytes()
        for repeat in (False, True):
            bodies = world_bodies(seed, solid, repeat, 1500)
            got, colour_shift, listed, _ = run_world(rules, tmp_path, blob, dims, info.columnCount, repeat, bodies_to_array(bodies))
            assert colour_shift == (2 if sparse else 7) and (sparse or listed > 0)
            want = model_results(solid, bodies, repeat)
            bad = np.flatnonzero(got != want)
            assert not len(bad), f"repeat {repeat}: {len(bad)} bodies differ; first {bodies[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
            assert (got["flags"] & RESTING).astype(bool).sum() > 100 and (got["flags"] & movemodel.BLOCKED[(0, 1)]).astype(bool).sum() > 20
    finally:
        ws.close()


# ---- hand-derived cases ----------------------------------------------------------------------------------------------------------------------------------

DIMS = (8, 16, 8)


def _floor(thick=2):
    solid = np.zeros(DIMS, dtype=bool)
    solid[:, :thick, :] = True
    return solid


def _move(rules, tmp_path, solid, b, repeat=False):
    """((x, y, z), flags) of one body from the rules AND from the model (they must agree)."""
    gx, dim_y, gz = solid.shape
    columns = []
    for x in range(gx):
        for z in range(gz):
            ys = np.nonzero(solid[x, :, z])[0][::-1]
            col = pyworld.final_column([(int(y), 0xFF000000 | int(y)) for y in ys], dim_y - 1, 1)
            columns.append((32 + 1000 * len(columns), list(col[0]), list(col[1])) if col else (32, [], []))
    got = _run_cases(rules, tmp_path, [(dim_y, gx, gz, 1, columns, repeat, [b])])[0][0]
    pos, flags = movemodel.move(solid, b, repeat)
    assert (list(got["pos"]), int(got["flags"])) == (pos, flags), (got, pos, flags)
    return tuple(pos), flags


def test_landing_flush_on_a_floor(rules, tmp_path):
    """The floor's top is y = 2 voxels = 512 units; a fall of 10 voxels from 5 voxels + 37 units ends there, blocked and resting."""
    b = movemodel.body((2 * U + 128, 5 * U + 37, 2 * U + 128), (128, U, 128), (0, -10 * U, 0))
    assert _move(rules, tmp_path, _floor(), b) == ((640, 512, 640), MINUS_Y | RESTING)
    # a fall that ends exactly on the floor is not blocked: moved = |d|
    b = movemodel.body((640, 5 * U + 37, 640), (128, U, 128), (0, -(3 * U + 37), 0))
    assert _move(rules, tmp_path, _floor(), b) == ((640, 512, 640), RESTING)


def test_a_stop_one_unit_short_of_the_request(rules, tmp_path):
    """A wall in slab x = 5 (1280 units); the box's +X face is at 768 + 200 = 968: 312 units are free.  A request of 313 is cut to 312 and sets
    the blocked bit; a request of 312 ends at the same place, flush and unblocked."""
    solid = _floor()
    solid[5, 2:10, :] = True
    at = (3 * U, 2 * U, 2 * U + 20)
    assert _move(rules, tmp_path, solid, movemodel.body(at, (200, U, 200), (313, 0, 0))) == ((1080, 512, 532), PLUS_X | RESTING)
    assert _move(rules, tmp_path, solid, movemodel.body(at, (200, U, 200), (312, 0, 0))) == ((1080, 512, 532), RESTING)
    # going -X towards a wall in slab 1 (its +X face at 512): from 768, 256 units are free
    solid[1, 2:10, :] = True
    assert _move(rules, tmp_path, solid, movemodel.body(at, (200, U, 200), (-257, 0, 0))) == ((512, 512, 532), MINUS_X | RESTING)


def _stair():
    solid = _floor()
    solid[5:, 2, :] = True  # one voxel high from x = 5 on
    return solid


def test_a_one_voxel_stair_is_climbed_with_step_up_256_and_refused_with_255(rules, tmp_path):
    """The box (+X face at 808 + 200 = 1008) walks 300 towards the stair at 1280: slide A stops after 272.  Raised by 256 it passes (y 768 .. 1167
    covers voxels 3 and 4) and walks the 300; the final -Y leg of 256 lands on the stair at once (slab 2 holds the stair under x = 5).
    Raised by 255 its bottom is at 767, still in voxel 2: blocked after 272 as well, not strictly farther, so A stands."""
    at, size = (3 * U + 40, 2 * U, 2 * U + 20), (200, 400, 200)
    assert _move(rules, tmp_path, _stair(), movemodel.body(at, size, (300, 0, 0), step_up=256)) == ((1108, 768, 532), MINUS_Y | STEPPED | RESTING)
    assert _move(rules, tmp_path, _stair(), movemodel.body(at, size, (300, 0, 0), step_up=255)) == ((1080, 512, 532), PLUS_X | RESTING)
    assert _move(rules, tmp_path, _stair(), movemodel.body(at, size, (300, 0, 0), step_up=0)) == ((1080, 512, 532), PLUS_X | RESTING)
    # with gravity in the same call: A's Y leg is blocked going down, which grounds the body; B's last leg is 256 + 30 long
    assert _move(rules, tmp_path, _stair(), movemodel.body(at, size, (300, -30, 0), step_up=256)) == ((1108, 768, 532), MINUS_Y | STEPPED | RESTING)
    # a two-voxel stair is too high for stepUp 256
    solid = _stair()
    solid[5:, 3, :] = True
    assert _move(rules, tmp_path, solid, movemodel.body(at, size, (300, 0, 0), step_up=256)) == ((1080, 512, 532), PLUS_X | RESTING)


def test_no_step_in_mid_air(rules, tmp_path):
    """100 units above the floor with delta_y = 0 the body is not resting: blocked by the stair, no step, however large stepUp is."""
    b = movemodel.body((3 * U + 40, 2 * U + 100, 2 * U + 20), (200, 400, 200), (300, 0, 0), step_up=4 * U)
    assert _move(rules, tmp_path, _stair(), b) == ((1080, 612, 532), PLUS_X)
    # rising does not step either
    b = movemodel.body((3 * U + 40, 2 * U, 2 * U + 20), (200, 400, 200), (300, 5, 0), step_up=4 * U)
    assert _move(rules, tmp_path, _stair(), b) == ((1080, 517, 532), PLUS_X)


def test_an_embedded_body_leaves(rules, tmp_path):
    """The box covers voxels y = 0 and 1 of the floor (200 .. 299): slabs it covers are never tested, the slabs above are free."""
    b = movemodel.body((2 * U + 10, 200, 2 * U + 10), (100, 100, 100), (0, 600, 0))
    assert _move(rules, tmp_path, _floor(), b) == ((522, 800, 522), STARTS_SOLID)
    # sideways inside the floor it is stopped by the next slab at once
    b = movemodel.body((2 * U + 10, 200, 2 * U + 10), (100, 100, 100), (500, 0, 0))
    assert _move(rules, tmp_path, _floor(), b) == ((2 * U + 156, 200, 522), STARTS_SOLID | PLUS_X)


def test_a_ledge_walked_off(rules, tmp_path):
    """A ledge x < 4 with its top at y = 6 voxels.  Three frames of (+200, -50): held by the ledge while any column of the footprint is over it,
    then over the edge (not resting any more), then the fall to the floor 4 voxels below."""
    solid = _floor()
    solid[:4, 2:6, :] = True
    size = (128, U, 128)
    assert _move(rules, tmp_path, solid, movemodel.body((3 * U, 6 * U, 2 * U), size, (200, -50, 0))) == ((968, 1536, 512), MINUS_Y | RESTING)
    assert _move(rules, tmp_path, solid, movemodel.body((968, 1536, 512), size, (200, -50, 0))) == ((1168, 1536, 512), MINUS_Y)
    assert _move(rules, tmp_path, solid, movemodel.body((1168, 1536, 512), size, (0, -2000, 0))) == ((1168, 512, 512), MINUS_Y | RESTING)


def test_solid_below_at_y_0(rules, tmp_path):
    """A hole through the floor at column (6, 6): with SOLID_BELOW the slab y = -1 stops the fall at 0, without it the body falls on."""
    solid = _floor()
    solid[6, :, 6] = False
    b = movemodel.body((6 * U + 50, 300, 6 * U + 50), (100, 100, 100), (0, -1000, 0))
    assert _move(rules, tmp_path, solid, dict(b, flags=movemodel.SOLID_BELOW)) == ((1586, 0, 1586), MINUS_Y | RESTING)
    assert _move(rules, tmp_path, solid, b) == ((1586, -700, 1586), 0)
    # a ground query below the world
    q = movemodel.body((1586, -256, 1586), (100, 100, 100), flags=movemodel.SOLID_BELOW)
    assert _move(rules, tmp_path, solid, q) == ((1586, -256, 1586), STARTS_SOLID | RESTING)


def test_wrapping_across_the_tile_edge(rules, tmp_path):
    """A wall in slab x = 0.  From x = 7 going +X, a repeating world meets it again in slab 8 (2048 units, 36 away from the face at 2012); the
    bounded world is air out there, or one solid wall with SOLID_SIDES."""
    solid = _floor()
    solid[0, 2:10, :] = True
    b = movemodel.body((7 * U + 20, 2 * U, 2 * U + 20), (200, U, 200), (300, 0, 0))
    assert _move(rules, tmp_path, solid, b, repeat=True) == ((1848, 512, 532), PLUS_X | RESTING)
    assert _move(rules, tmp_path, solid, b) == ((2112, 512, 532), 0)
    assert _move(rules, tmp_path, solid, dict(b, flags=movemodel.SOLID_SIDES)) == ((1848, 512, 532), PLUS_X | RESTING)
    assert _move(rules, tmp_path, solid, dict(b, flags=movemodel.SOLID_SIDES), repeat=True) == ((1848, 512, 532), PLUS_X | RESTING)
    # -Z across z = 0 into the floorless copy?  The floor repeats too: the body rests at z < 0
    c = movemodel.body((3 * U, 2 * U, 20), (200, U, 200), (0, 0, -300))
    assert _move(rules, tmp_path, solid, c, repeat=True) == ((768, 512, -280), RESTING)
    assert _move(rules, tmp_path, solid, c) == ((768, 512, -280), 0)


# ---- layouts and entry points ----------------------------------------------------------------------------------------------------------------------------

def test_move_fails_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    b, r = gpu.MoveBody(), gpu.MoveResult()
    b.size[0] = b.size[1] = b.size[2] = 1
    assert L.cvx_world_move(None, 1, C.byref(b), C.byref(r)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    assert L.cvx_world_move_device(None, 1, C.byref(b), C.byref(r), 0, None) == -1
    # a context without a device or world (tests/move_rules.cpp): the host-array call's 5 pointer / count cases and 13 body limits, the device
    # call's 4 and 7 values of lanesPerBody that are not 0, 1, 4, 16, 64: all INVALID_ARGUMENT; then six valid calls: NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 29 + [-3] * 6, codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_move(h, 1, C.byref(b), C.byref(r)) == -3
            assert L.cvx_world_move_device(h, 1, C.byref(b), C.byref(r), 16, None) == -3
        finally:
            L.cvx_destroy(h)


def test_bodies_outside_the_limits_come_back_invalid_from_the_rule(rules, tmp_path):
    """What the kernel answers for input the device call cannot check on the host: pos unchanged, CVX_MOVED_INVALID, nothing walked."""
    bad = [movemodel.body((5, 6, 7), (0, 1, 1)), movemodel.body((5, 6, 7), (1, 64 * U + 1, 1)), movemodel.body((5, 6, 7), (1, 1, 1), (0, 0, 256 * U + 1)),
           movemodel.body((5, 6, 7), (1, 1, 1), step_up=4 * U + 1), movemodel.body((5, 6, 7), (1, 1, 1), step_up=-1), movemodel.body((5, 6, 7), (1, 1, 1), flags=4),
           movemodel.body((2**28 + 1, 6, 7), (1, 1, 1)), movemodel.body((5, -2**31, 7), (1, 1, 1), (0, -2**31, 0))]
    got = _run_cases(rules, tmp_path, [(8, 1, 1, 1, [(32, [], [])], False, bad)])[0]
    for b, r in zip(bad, got):
        assert list(r["pos"]) == b["pos"] and int(r["flags"]) == movemodel.INVALID
        assert movemodel.move(np.zeros((1, 8, 1), dtype=bool), b) == (b["pos"], movemodel.INVALID)
