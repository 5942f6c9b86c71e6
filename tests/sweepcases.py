"""The cases of cvxs_world_sweep that tests/test_world_sweep_cpu.py runs through the host rules and tests/test_gpu_world_sweep.py through the
device, and the answer of tests/sweepmodel.py for each, computed once.

  world(key)   -> (dims, solid, colour) of "thin" (a 32^3 world whose floor is one voxel thick, with a hole), "walled" (the flat 32^3 world with a
                  wall), "tall" (the 32 x 256 x 32 world with a comb column of 40 runs) and "terrain" (128 x 64 x 128)
  CASES        -> name: a function that gives (world key, models, instances, motions, solid_outside)
  case(name), answer(name) -> the case and the model's (sweeps, contacts, points, summary with jobs), both cached"""
from __future__ import annotations

import functools

import numpy as np

import sweepmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _dense
from test_gpu_world_dense import TALL, _tall_solid
from test_gpu_world_edit import DIMS, _terrain
from test_world_contacts_cpu import CUBE, colour_of, cube_model, flat_world
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, random_model, rotation, tilt

DEFAULT = gpu.SURFACE_OUTSIDE_DEFAULT
FLAT = (32, 32, 32)
FLOOR = 10             # "thin": the floor's one layer
COMB = (5, 5)          # "tall": the column of 40 runs of two voxels, two voxels apart, from y = 20
COMB_RUNS = 40
PLATE, VOXEL = (8, 1, 8), (1, 1, 1)


@functools.lru_cache(maxsize=None)
def world(key):
    if key == "thin":
        solid = np.zeros(FLAT, dtype=bool)
        solid[:, FLOOR, :] = True
        solid[24:, FLOOR, 24:] = False  # empty columns
        return FLAT, solid, colour_of(solid)
    if key == "walled":
        return (FLAT, *flat_world(wall=True, dims=FLAT))
    if key == "tall":
        solid = _tall_solid()
        solid[COMB[0], :, COMB[1]] = False
        for i in range(COMB_RUNS):
            solid[COMB[0], 20 + 4 * i:22 + 4 * i, COMB[1]] = True
        return TALL, solid, _dense(solid)
    assert key == "terrain"
    solid = _terrain()
    return DIMS, solid, _dense(solid)


def _full(size, argb=0xFF445566):
    return (np.full((size[0], size[2], size[1]), argb, dtype=np.uint32), None)


def _only(size, ys):
    """A model of `size` whose set voxels are the heights `ys` of its column (0, 0)."""
    argb = np.zeros((size[0], size[2], size[1]), dtype=np.uint32)
    argb[0, 0, list(ys)] = 0xFF99AA11
    return (argb, None)


def _top(solid, x, z):
    ys = np.nonzero(solid[x, :, z])[0]
    return int(ys.max()) if len(ys) else -1


def _plate(y, motion, so=DEFAULT):
    return "thin", [_full(PLATE)], [identity_at((12, y, 12), PLATE, 0, gpu.BRUSH_FILL)], [motion], so


def _cube(world_key, at, motion, so):
    return world_key, [cube_model()], [identity_at(at, CUBE, 0, gpu.BRUSH_FILL)], [motion], so


def _column(height, motion_y):
    """A full column of `height` voxels over the tall world's ground, its lowest voxel `abs(motion_y) - 2` above the ground's top."""
    _, solid, _ = world("tall")
    x, z = 20, 1
    assert (x // 2 + z // 3) % 5 == 0 and _top(solid, x, z) == 63, "a column with the slab [40, 64)"
    size = (1, height, 1)
    return "tall", [_full(size)], [identity_at((x, 64 + abs(motion_y) - 2, z), size, 0, gpu.BRUSH_FILL)], [(0, motion_y, 0)], DEFAULT


def _lane(lane):
    """A 64-voxel box whose only body voxel is lane `lane` of its one step (lane 0 the top), falling onto the tall world's slab."""
    size = (1, 64, 1)
    return "tall", [_only(size, [63 - lane])], [identity_at((20, 70, 1), size, 0, gpu.BRUSH_FILL)], [(0, -80, 0)], DEFAULT


def _comb():
    models = [_full(VOXEL)]
    instances, motions = [], []
    for i in range(COMB_RUNS):  # run i is y = 20 + 4 i, 21 + 4 i: down onto it from the top of the gap above it, up into it from the bottom of the gap below it
        instances += [identity_at((COMB[0], 23 + 4 * i, COMB[1]), VOXEL, 0, gpu.BRUSH_FILL), identity_at((COMB[0], 18 + 4 * i, COMB[1]), VOXEL, 0, gpu.BRUSH_FILL)]
        motions += [(0, -3 - i % 3, 0), (0, 3 + i % 2, 0)]
    return "tall", models, instances, motions, 0


MAPS = {"yaw 30": rotation(1, 30), "tilt": tilt(), "scale 2": 2 * rotation(1, 30), "scale 1/2": 0.5 * np.eye(3)}


def _maps():
    _, solid, _ = world("terrain")
    size = (9, 11, 7)
    models = [random_model(np.random.default_rng(77), size, zeros=0.3)]
    instances, motions = [], []
    for k, (name, linear) in enumerate(MAPS.items()):
        cx, cz = 30 + 20 * k, 40 + 13 * k
        for v in ((0, -30, 0), (5, -14, -3), (-4, 9, 6)):
            start = (cx, 33 if v[1] > 0 else 58, cz) if name == "scale 2" else (cx, 30 if v[1] > 0 else 46, cz)
            instances.append(gpu.model_instance(forward_about_centre(linear, size, start), size, 0, gpu.BRUSH_FILL))
            motions.append(v)
    return "terrain", models, instances, motions, DEFAULT


def _many(count, distinct, seed):
    """`count` one-voxel instances over the terrain, drawn from `distinct` (position, motion) pairs."""
    rng = np.random.default_rng(seed)
    _, solid, _ = world("terrain")
    pool = []
    for _ in range(distinct):
        x, z = int(rng.integers(4, DIMS[0] - 4)), int(rng.integers(4, DIMS[2] - 4))
        y = _top(solid, x, z) + int(rng.integers(1, 6))
        pool.append(((x, y, z), (int(rng.integers(-3, 4)), int(rng.integers(-7, 3)), int(rng.integers(-3, 4)))))
    picks = rng.integers(0, distinct, size=count)
    return ("terrain", [_full(VOXEL)], [identity_at(pool[p][0], VOXEL, 0, gpu.BRUSH_FILL) for p in picks], [pool[p][1] for p in picks], DEFAULT)


CASES = {
    # the thin shell and the ends of the range
    "thin shell": lambda: _plate(FLOOR + 5, (0, -12, 0)),
    "starts solid": lambda: _plate(FLOOR, (0, -3, 0)),
    "hit at n": lambda: _plate(FLOOR + 5, (0, -5, 0)),
    "miss by one": lambda: _plate(FLOOR + 5, (0, -4, 0)),
    "still": lambda: ("thin", [_full(PLATE)], [identity_at((12, FLOOR + 5, 12), PLATE, 0, 0), identity_at((12, FLOOR, 12), PLATE, 0, 0)], [(0, 0, 0), (0, 0, 0)], DEFAULT),
    # every axis and sign
    "-x": lambda: _cube("walled", (10, 12, 14), (-7, 0, 0), DEFAULT),
    "+x": lambda: _cube("walled", (26, 12, 14), (8, 0, 0), DEFAULT | 0x02),
    "+x open": lambda: _cube("walled", (26, 12, 14), (8, 0, 0), DEFAULT),
    "-y": lambda: _cube("walled", (14, 12, 14), (0, -9, 0), DEFAULT),
    "+y": lambda: _cube("walled", (14, 26, 14), (0, 9, 0), DEFAULT | 0x08),
    "-z": lambda: _cube("walled", (14, 12, 2), (0, 0, -6), DEFAULT | 0x10),
    "+z": lambda: _cube("walled", (14, 12, 26), (0, 0, 7), DEFAULT | 0x20),
    "3 -1 2": lambda: _cube("walled", (27, 8, 14), (3, -1, 2), DEFAULT | 0x02),
    "2 2 2": lambda: _cube("walled", (27, 27, 27), (2, 2, 2), 0x2E),
    "-5 7 -3": lambda: _cube("walled", (8, 10, 1), (-5, 7, -3), DEFAULT | 0x10),
    # outside the world
    "below the world": lambda: ("thin", [_full(VOXEL)], [identity_at((27, 6, 27), VOXEL, 0, 0)], [(0, -10, 0)], DEFAULT),
    "sideways": lambda: ("thin", [_full(VOXEL)], [identity_at((29, 20, 3), VOXEL, 0, 0), identity_at((3, 20, 29), VOXEL, 0, 0)], [(6, 1, -6), (-6, -1, 6)], 0x33),
    "sideways open": lambda: ("thin", [_full(VOXEL)], [identity_at((29, 20, 3), VOXEL, 0, 0), identity_at((3, 20, 29), VOXEL, 0, 0)], [(6, 1, -6), (-6, -1, 6)], 0),
    # waves
    "column 65": lambda: _column(65, -6),
    "column 200": lambda: _column(200, -9),
    "column 300": lambda: _column(300, -4),
    "lane 0": lambda: _lane(0),
    "lane 63": lambda: _lane(63),
    # the binary search
    "comb": _comb,
    # maps
    "maps": _maps,
    # many jobs
    "65 instances": lambda: _many(65, 65, 1),
    "4096 instances": lambda: _many(4096, 96, 2),
    "8193 stations": lambda: ("terrain", [_full(VOXEL)], [identity_at((64, 40, 64), VOXEL, 0, 0)], [(4096, -3, -4096)], 0x3F),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def answer(name):
    key, models, instances, motions, so = case(name)
    _, solid, colour = world(key)
    dicts = as_dicts(instances)
    sweeps, contacts, points, summary = sweepmodel.sweep(solid, colour, models, dicts, motions, so)
    summary["jobs"] = sweepmodel.jobs(dicts, motions)
    return sweeps, contacts, points, summary
