"""The cases of cvxd_models_brush that tests/test_model_brush_cpu.py runs through the host rules and tests/test_gpu_model_brush.py through the
device, and the answer of tests/modelbrushmodel.py for each, computed once.

  CASES        -> name: a function that gives (models, instances, strokes)
  case(name), answer(name) -> the case and the model's (models after, model results, instance results, summary), both cached and never changed
  property_of(name)        -> asserts, from the model's answer alone, the property the case is named for"""
from __future__ import annotations

import functools

import numpy as np

import modelbrushmodel
from cpuvox_amd import gpu
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, make_instance, random_model, rotation, tilt

CARVE, PAINT = gpu.BRUSH_CARVE, gpu.BRUSH_PAINT
BOX, SPHERE, CAPSULE, ELLIPSOID = gpu.SHAPE_BOX, gpu.SHAPE_SPHERE, gpu.SHAPE_CAPSULE, gpu.SHAPE_ELLIPSOID
ONE = 65536
COLUMNS = (63, 64, 65, 129)
RED, GREEN, BLUE = 0xFFCC2211, 0xFF22CC11, 0xFF1122CC


def _full(size, argb=0xFF445566, mask=False, colours=True):
    shape = (size[0], size[2], size[1])
    return (np.full(shape, argb, dtype=np.uint32) if colours else None, np.ones(shape, dtype=bool) if mask else None)


def _ramp(size):
    """Every voxel set, every colour its own: a moved or lost voxel shows."""
    n = size[0] * size[1] * size[2]
    return ((0xFF000000 + 1 + np.arange(n, dtype=np.uint32)).reshape(size[0], size[2], size[1]), None)


def box(op, lo, hi, argb=0):
    return dict(op=op, shape=BOX, a=list(lo), b=list(hi), argb=argb)


def sphere(op, centre, radius, argb=0):
    return dict(op=op, shape=SPHERE, a=list(centre), b=[radius, 0, 0], argb=argb)


def capsule(op, a, b, radius, argb=0):
    return dict(op=op, shape=CAPSULE, a=list(a), b=list(b), radius=radius, argb=argb)


def ellipsoid(op, centre, radii, argb=0):
    return dict(op=op, shape=ELLIPSOID, a=list(centre), b=list(radii), argb=argb)


def _placed(linear, size, centre, model=0):
    return gpu.model_instance(forward_about_centre(linear, size, centre), size, model, gpu.BRUSH_FILL)


# ---- step edges -------------------------------------------------------------------------------------------------------------------------------------

def _column(height):
    """A full column of `height` voxels in a box as tall, top voxel at y = 10 + height - 1 (lane 0 of the first step).  A sphere of one voxel at
    the top, a box on the lowest voxel, a box across the step boundary 64 below the top where there is one, and a PAINT of the whole column
    below them in the list."""
    size = (1, height, 1)
    top = 10 + height - 1
    strokes = [box(PAINT, (3, 0, 3), (4, 1000, 4), GREEN), sphere(CARVE, (3, top, 3), 0), box(CARVE, (3, 10, 3), (4, 11, 4))]
    if height > 64:
        strokes.append(box(CARVE, (3, top - 64, 3), (4, top - 62, 4)))  # lane 63 of step 0 and lane 0 of step 1
    return [_ramp(size)], [identity_at((3, 10, 3), size)], strokes


def _tall_box():
    """A body of five voxels in a box 300 tall: the cut leaves the steps that can hold it.  One voxel carved, one painted."""
    size = (1, 5, 1)
    inst = make_instance(np.eye(3, dtype=np.int64) * ONE, [-2 * ONE, -140 * ONE, -2 * ONE], (2, 0, 2), (3, 300, 3))
    return [_ramp(size)], [inst], [box(CARVE, (2, 141, 2), (3, 142, 2 + 1)), sphere(PAINT, (2, 144, 2), 0, RED), box(CARVE, (2, 200, 2), (3, 290, 3))]


def _lanes():
    """A 2 x 128 x 1 body, top voxel at y = 127: spans that begin or end on lane 0 and lane 63 of both steps, one of exactly one voxel in the
    middle of a step, and a sphere whose footprint meets the box and column x = 1 but whose span misses it (only column x = 0 is cut)."""
    size = (2, 128, 1)
    strokes = [box(CARVE, (0, 127, 0), (1, 128, 1)), box(PAINT, (0, 64, 0), (1, 65, 1), RED), box(CARVE, (0, 63, 0), (1, 64, 1)), box(PAINT, (0, 0, 0), (1, 1, 1), GREEN),
               box(CARVE, (1, 100, 0), (2, 101, 1)), box(PAINT, (1, 60, 0), (2, 68, 1), BLUE), capsule(CARVE, (-3, 30, 0), (0, 30, 0), 0)]
    return [_ramp(size)], [identity_at((0, 0, 0), size)], strokes


def _misses():
    """A sphere whose footprint box covers column (2, 2) of the body and whose span there is empty (9 + 9 > 9); column (3, 3) is cut (4 + 4 <= 9)."""
    size = (4, 9, 4)
    return [_ramp(size)], [identity_at((0, 0, 0), size)], [sphere(CARVE, (5, 4, 5), 3)]


# ---- maps -------------------------------------------------------------------------------------------------------------------------------------------

MAPS = {"translated": np.eye(3), "rotated 90": rotation(1, 90), "yaw 30": rotation(1, 30), "magnified 2": 2.0 * np.eye(3), "minified 1/2": 0.5 * np.eye(3),
        "tilt": tilt()}


def _map(name, centre=(20.3, 15.1, 17.6)):
    rng = np.random.default_rng(5 + sorted(MAPS).index(name))
    size = (7, 9, 6)
    model = random_model(rng, size, with_mask=True, zeros=0.25)
    c = [int(v) for v in centre]
    strokes = [sphere(PAINT, (c[0] + 2, c[1], c[2]), 4, RED), sphere(CARVE, (c[0] - 2, c[1] + 1, c[2] + 1), 3), box(PAINT, (c[0] - 9, c[1] - 1, c[2] - 9), (c[0] + 9, c[1] + 1, c[2] + 9), BLUE)]
    return [model], [_placed(MAPS[name], size, np.asarray(centre))], strokes


def _negative():
    return _map("yaw 30", centre=(-1000.4, -37.2, -5.5))


# ---- folds ------------------------------------------------------------------------------------------------------------------------------------------

def _fold(ops):
    """One voxel at (5, 5, 5) under the listed ops, in order, each a sphere of that voxel alone (PAINT j has colour 0xFF000001 + j)."""
    strokes = [sphere(op, (5, 5, 5), 0, 0xFF000001 + j if op == PAINT else 0) for j, op in enumerate(ops)]
    return [_full((1, 1, 1), mask=True)], [identity_at((5, 5, 5), (1, 1, 1))], strokes


def _two_instances():
    """Two instances of one 4 x 4 x 4 model far apart, hit by different strokes: the model takes both."""
    size = (4, 4, 4)
    return [_ramp(size)], [identity_at((0, 0, 0), size), identity_at((100, 0, 0), size)], [box(CARVE, (0, 0, 0), (1, 4, 4)), box(PAINT, (103, 0, 0), (104, 4, 4), RED),
                                                                                            box(CARVE, (102, 3, 0), (104, 4, 4))]


def _same_voxel():
    """Two instances of one model through different maps -- as it lies, and turned 90 degrees about y -- hit on the SAME model voxel: a PAINT
    through the first, a later CARVE through the second."""
    size = (3, 3, 3)
    turned = _placed(rotation(1, 90), size, np.array([51.5, 1.5, 1.5]))
    model = _ramp(size)
    d = None
    for x in range(50, 53):  # the voxel of the turned instance whose image is model voxel (0, 1, 2)
        for z in range(0, 3):
            s = modelbrushmodel.modelsmodel.apply_map(*[as_dicts([turned])[0][k] for k in ("m", "t")], np.array([x, 1, z]))
            if s.tolist() == [0, 1, 2]:
                d = (x, 1, z)
    assert d is not None
    return [model], [identity_at((0, 0, 0), size), turned], [sphere(PAINT, (0, 1, 2), 0, RED), sphere(CARVE, d, 0), sphere(PAINT, (2, 2, 2), 0, GREEN)]


# ---- models and shapes ------------------------------------------------------------------------------------------------------------------------------

def _kinds():
    """A mask alone (PAINT ignored, its counts 0), colours alone and both, side by side under the same two strokes."""
    size = (5, 5, 5)
    rng = np.random.default_rng(3)
    both = random_model(rng, size, with_mask=True, zeros=0.2)
    models = [(None, np.array(both[1])), (np.where(both[1], both[0] | 0xFF000000, 0).astype(np.uint32), None), both]
    instances = [identity_at((10 * g, 0, 0), size, g) for g in range(3)]
    return models, instances, [box(PAINT, (0, 0, 0), (30, 3, 5), RED), box(CARVE, (0, 2, 0), (30, 4, 2))]


SHAPES = {"box": lambda op, c, argb=0: box(op, (c[0] - 3, c[1] - 1, c[2] - 2), (c[0] + 2, c[1] + 3, c[2] + 4), argb),
          "sphere": lambda op, c, argb=0: sphere(op, c, 4, argb),
          "capsule": lambda op, c, argb=0: capsule(op, (c[0] - 5, c[1] - 3, c[2] - 1), (c[0] + 4, c[1] + 2, c[2] + 3), 2, argb),
          "ellipsoid": lambda op, c, argb=0: ellipsoid(op, c, (6, 2, 4), argb)}


def _shape(name):
    rng = np.random.default_rng(11)
    size = (9, 10, 8)
    centre = (30, 22, 14)
    strokes = [SHAPES[name](PAINT, (centre[0] + 1, centre[1] + 1, centre[2]), RED), SHAPES[name](CARVE, (centre[0] - 2, centre[1] - 1, centre[2] + 1))]
    return [random_model(rng, size, zeros=0.2)], [_placed(tilt(), size, np.array([30.4, 22.2, 14.9]))], strokes


# ---- nothing hit, twice -----------------------------------------------------------------------------------------------------------------------------

def _far():
    models, instances, _ = _map("tilt")
    return models, instances, [sphere(CARVE, (500, 500, 500), 20), capsule(PAINT, (600, 0, 0), (610, 5, 5), 3, RED)]


def _near_miss():
    """The strokes' reach meets the box (the instance has jobs), the strokes themselves touch no body voxel."""
    size = (4, 4, 4)
    model = _ramp(size)
    model[0][0, :, :] = 0
    return [model], [identity_at((0, 0, 0), size)], [box(CARVE, (0, 0, 0), (1, 4, 4)), box(PAINT, (-3, 0, 0), (0, 4, 4), RED)]


# ---- limits -----------------------------------------------------------------------------------------------------------------------------------------

def _many_strokes():
    """4096 strokes on one body: every list word in use; single voxels, PAINTs and CARVEs interleaved, each voxel hit up to three times."""
    size = (16, 16, 8)
    strokes = []
    for j in range(4096):
        v = (j * 7) % 2048
        at = (v // 128, (v // 8) % 16, v % 8)
        strokes.append(sphere(CARVE if j % 5 == 4 else PAINT, at, 0, 0 if j % 5 == 4 else 0xFF100000 + j))
    return [_ramp(size)], [identity_at((0, 0, 0), size)], strokes


def _many_instances():
    """4096 instances of 1 - 3-voxel models (three models, shared), one box stroke over a third of them and one sphere in the middle."""
    models = [_ramp((1, n, 1)) for n in (1, 2, 3)]
    instances = [identity_at((2 * (k % 64), 4 * (k // 64 % 8), 2 * (k // 512)), (1, 1 + k % 3, 1), k % 3) for k in range(4096)]
    return models, instances, [box(PAINT, (0, 0, 0), (128, 40, 5), BLUE), sphere(CARVE, (64, 16, 8), 9)]


def _many_models():
    """256 models of their own, a row of bodies, one sphere through the middle of the row and one stroke hitting all of them."""
    rng = np.random.default_rng(19)
    models = [random_model(rng, (2 + g % 3, 3, 2), with_mask=g % 2 == 0, zeros=0.2) for g in range(256)]
    instances = [identity_at((5 * g, 0, 0), (2 + g % 3, 3, 2), g) for g in range(256)]
    return models, instances, [box(PAINT, (-5, 0, 0), (1300, 3, 2), GREEN), sphere(CARVE, (640, 1, 1), 30)]


CASES = {f"column {h}": functools.partial(_column, h) for h in COLUMNS}
CASES.update({"tall box": _tall_box, "lanes": _lanes, "misses": _misses, "negative": _negative, "two instances": _two_instances, "same voxel": _same_voxel,
              "kinds": _kinds, "far": _far, "near miss": _near_miss, "paint carve paint": functools.partial(_fold, (PAINT, CARVE, PAINT)),
              "paint paint": functools.partial(_fold, (PAINT, PAINT, PAINT)), "carve": functools.partial(_fold, (CARVE,)), "4096 strokes": _many_strokes,
              "4096 instances": _many_instances, "256 models": _many_models})
CASES.update({f"map {name}": functools.partial(_map, name) for name in MAPS})
CASES.update({f"shape {name}": functools.partial(_shape, name) for name in SHAPES})


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def answer(name):
    models, instances, strokes = case(name)
    return modelbrushmodel.brush(models, as_dicts(instances), strokes)


def property_of(name):
    models, instances, strokes = case(name)
    after, results, hit, summary = answer(name)
    if name.startswith("column"):
        h = int(name.split()[1])
        top = 10 + h - 1
        assert results["carved"][0] == len({top, 10} | ({top - 64, top - 63} if h > 64 else set())) and results["voxels"][0] == h - results["carved"][0] == results["painted"][0]
        assert hit["carved"][0] == results["carved"][0] and hit["painted"][0] == h - hit["carved"][0] and summary["jobs"] == 1
    elif name == "tall box":
        assert results[0]["carved"] == 1 and results[0]["painted"] == 1 and results[0]["voxels"] == 4 and after[0][0][0, 0, 4] == RED and after[0][0][0, 0, 1] == 0
    elif name == "lanes":
        argb = after[0][0]
        assert [int(argb[0, 0, y]) for y in (127, 64, 63, 0)] == [0, RED, 0, GREEN] and argb[0, 0, 30] == 0 and argb[1, 0, 30] != 0 and argb[1, 0, 100] == 0
        assert results[0]["carved"] == 4 and results[0]["painted"] == 2 + 8
    elif name == "misses":
        argb = after[0][0]
        assert (argb[2, 2, :] != 0).all() and argb[3, 3, 4] == 0 and argb[3, 3, 6] != 0 and results[0]["carved"] > 0 and summary["jobs"] == 16
    elif name.startswith("map") or name == "negative":
        assert results[0]["carved"] > 0 and results[0]["painted"] > 0 and hit[0]["carved"] > 0
        if name == "map magnified 2":
            assert hit[0]["carved"] > results[0]["carved"], "many d to one s"
        if name == "map minified 1/2":
            inst = as_dicts(instances)[0]
            _, inside, at = modelbrushmodel._images(models[0], inst)
            reached = np.zeros(models[0][0].shape, dtype=bool)
            reached[tuple(a[inside] for a in at)] = True
            assert not reached.all() and (after[0][0][~reached] == models[0][0][~reached]).all() and (after[0][1][~reached] == (models[0][1][~reached] != 0)).all()
    elif name in ("paint carve paint", "carve"):
        assert results[0]["voxels"] == 0 and results[0]["carved"] == 1 and results[0]["painted"] == 0 and not after[0][1].any() and not after[0][0].any()
        assert results[0]["min"].tolist() == results[0]["max"].tolist() == [0, 0, 0] and hit[0].tolist() == (1, 0)
    elif name == "paint paint":
        assert after[0][0][0, 0, 0] == 0xFF000003 and results[0]["painted"] == 1 and hit[0].tolist() == (0, 1)
    elif name == "two instances":
        argb = after[0][0]
        assert not argb[0].any() and (argb[3, :, :3] == RED).all() and not argb[2:, :, 3].any() and hit["carved"].tolist() == [16, 8]
    elif name == "same voxel":
        assert after[0][0][0, 2, 1] == 0 and after[0][0][2, 2, 2] == GREEN and results[0]["carved"] == 1 and results[0]["painted"] == 1
        assert hit[0].tolist() == (0, 2) and hit[1]["carved"] == 1
    elif name == "kinds":
        assert results["painted"][0] == 0 and hit["painted"][0] == 0 and results["carved"][0] == results["carved"][1] == results["carved"][2] > 0
        assert results["painted"][1] == results["painted"][2] > 0 and (after[0][1] == after[2][1]).all() and after[0][0] is None and after[1][1] is None
    elif name in ("far", "near miss"):
        assert summary["carved"] == summary["painted"] == summary["models"] == 0 and results["voxels"][0] > 0 and results["max"][0].max() > 0
        assert (after[0][0] == models[0][0]).all() and summary["jobs"] == (0 if name == "far" else 16) and not hit["carved"].any() and not hit["painted"].any()
    elif name == "4096 strokes":
        assert len(strokes) == 4096 and results[0]["carved"] > 300 and results[0]["painted"] > 1000
    elif name == "4096 instances":
        assert len(instances) == 4096 and (hit["carved"] > 0).sum() > 20 and (hit["painted"] > 0).sum() > 1000 and summary["models"] == 3
    elif name == "256 models":
        assert len(models) == 256 and summary["models"] == 256 and (results["carved"] > 0).sum() > 5
    elif name.startswith("shape"):
        assert results[0]["carved"] > 10 and results[0]["painted"] > 5
    else:
        raise AssertionError(name)
