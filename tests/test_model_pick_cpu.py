"""CPU (no GPU needed): the rules behind cvxq_model_pick (cpuvox_amd/csrc/cvx_model_pick.h), compiled for the host through
tests/model_pick_rules.cpp, against the independent numpy model of tests/modelpickmodel.py.  The program runs the sequential pair rule (a voxel
at a time, the nearest body by the floats) AND the kernels' walk (a wave per job, 64 layers a step, lane after lane, the key's minimum, the
second walk of the winner) and fails when they differ in a byte of any job or any hit.

- The scene of the GPU test (tests/test_gpu_model_pick.py builds it here): three models, eight instances under rotations, scales and a mirror,
  4096 rays; the rules equal the model on every unambiguous ray, and at least 0.99 of the rays are unambiguous.
- The adversarial rays (voxel corners and edges, equal |d| on two and three axes, zeros, origins on the box, maxT an ulp around the hit, +inf,
  a zero direction, NaN, inf, a negative maxT) with the outputs the contract defines, by hand.
- The steps of the walk: boxes 1 .. 200 layers long on every axis and sign with the body's only voxel in layers 0 .. 128.
- The ray rule: five bodies in a line, the list permuted, two identical instances.
- Every argument check with its message, the wrappers' checks, and the same stand-alone program under -fsanitize=address,undefined."""
import functools
import subprocess

import numpy as np
import pytest

import modelpickmodel
import pickmodel
import ruleslib
from cpuvox_amd import gpu
from test_world_contacts_cpu import CUBE, SANITIZE, cube_model
from test_world_models_cpu import as_dicts, call_words, forward_about_centre, identity_at, make_instance, random_model, rotation, tilt

FILL = gpu.BRUSH_FILL
ONE = 1 << 16
INF, NAN = np.float32(np.inf), np.float32(np.nan)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("model_pick"))


# ---- building calls (the GPU test uses these too) -----------------------------------------------------------------------------------------------

def rays_of(origins, directions, max_t):
    o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
    rays = np.zeros(len(o), dtype=gpu.PICK_RAY_DTYPE)
    rays["origin"], rays["direction"] = o, np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    rays["maxT"] = np.broadcast_to(np.asarray(max_t, dtype=np.float32), (len(o),))
    return rays


def case_words(models, instances, rays):
    return [call_words(models, instances), [len(rays)], np.ascontiguousarray(rays).view(np.int32).ravel()]


def run_cases(rules, tmp_path, cases):
    """[(models, instances, rays)] -> [(hits as MODEL_HIT_DTYPE, jobs)]: the program fails when the wave's walk differs from the rule."""
    parts = [p for case in cases for p in case_words(*case)]
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *parts, dtype=np.uint8)
    out, at = [], 0
    for _, _, rays in cases:
        n = len(rays) * gpu.MODEL_HIT_DTYPE.itemsize
        out.append((raw[at:at + n].view(gpu.MODEL_HIT_DTYPE).copy(), int(raw[at + n:at + n + 8].view(np.int64)[0])))
        at += n + 8
    assert at == len(raw)
    return out


def ball_model(n=16):
    """(n, n, n), a solid ball, argb only with 0 as air."""
    c = (np.arange(n) + 0.5 - n / 2) ** 2
    inside = c[:, None, None] + c[None, :, None] + c[None, None, :] <= (n / 2) ** 2
    return np.where(inside, np.uint32(0xFF4060A0) + np.arange(n, dtype=np.uint32)[None, None, :], np.uint32(0)).astype(np.uint32), None


SCENE_DIMS = (72, 48, 72)


@functools.lru_cache(maxsize=None)
def scene():
    """(models, instances, rays, the model's answer): three models, eight instances, 4096 rays, half of them pickmodel.random_rays over
    SCENE_DIMS and half aimed at random points of the instances' boxes.  Several boxes overlap, one reaches below y = 0, one below x = 0."""
    rng = np.random.default_rng(2026)
    sizes = [(12, 9, 7), (16, 16, 16), (5, 20, 6)]
    models = [random_model(rng, sizes[0], with_mask=True, zeros=0.5), ball_model(), (None, np.ones((5, 6, 20), dtype=bool))]
    specs = [(0, np.eye(3), (20, 10, 20)), (1, rotation(1, 30), (30, 12, 26)), (0, tilt(), (36, 20, 30)), (2, rotation(0, 40) @ rotation(2, 65), (44, 14, 40)),
             (1, 0.5 * np.eye(3), (24, 6, 30)), (0, 1.5 * rotation(1, 15), (50, 3, 22)), (2, 2.0 * rotation(2, 20), (4, 24, 50)),
             (0, rotation(1, 10) @ np.diag([1.0, 1.0, -1.0]), (28, 14, 34))]
    instances = [gpu.model_instance(forward_about_centre(linear, sizes[m], centre), sizes[m], m, FILL) for m, linear, centre in specs]
    n = 4096
    o1, d1, t1 = pickmodel.random_rays(rng, SCENE_DIMS, n // 2)
    o2 = rng.uniform(-0.3, 1.3, size=(n // 2, 3)) * np.array(SCENE_DIMS, dtype=np.float64)
    which = rng.integers(0, len(instances), size=n // 2)
    lo = np.array([list(instances[k].boxMin) for k in which], dtype=np.float64)
    hi = np.array([list(instances[k].boxMax) for k in which], dtype=np.float64)
    d2 = lo + rng.uniform(0.0, 1.0, size=(n // 2, 3)) * (hi - lo) - o2
    t2 = np.where(rng.integers(0, 6, size=n // 2) == 0, rng.uniform(0.05, 0.9, size=n // 2), 1e4)
    rays = rays_of(np.concatenate([o1, o2]), np.concatenate([d1, d2]), np.concatenate([t1, t2]))
    model = modelpickmodel.pick_many(models, as_dicts(instances), rays["origin"], rays["direction"], rays["maxT"])
    return models, instances, rays, model


def wide_cube():
    """The 4 x 4 x 4 cube at (10, 10, 10) in a box three voxels wider on every side: (models, instances)."""
    return [cube_model()], [make_instance(np.eye(3, dtype=np.int64) * ONE, [-10 * ONE] * 3, [7] * 3, [17] * 3, 0, FILL)]


def below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def above(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


# (origin, direction, maxT, the hit by hand: (voxel, face, t) or None for a miss)
ADVERSARIAL = [
    # integral origins, diagonals through voxel corners and edges: the lower axis crosses first, the last crossing names the face
    ((5, 5, 5), (1, 1, 1), 100, ((10, 10, 10), 4, 5.0)),
    ((5, 19, 12), (1, -1, 0), 100, ((10, 13, 12), 3, 5.0)),
    ((19, 5, 19), (-1, 1, -1), 100, ((13, 10, 13), 5, 5.0)),
    ((5, 5, 12), (1, 1, 0), 100, ((10, 10, 12), 2, 5.0)),
    ((12, 19, 19), (0, -1, -1), 100, ((12, 13, 13), 5, 5.0)),
    # |d| equal on two and on three axes, off the grid
    ((5.25, 5.5, 5.75), (1, 1, 1), 100, ((10, 10, 10), 0, 4.75)),
    ((5.25, 12.5, 5.5), (2, 0.5, 2), 100, ((10, 13, 10), 0, 2.375)),
    # a zero in one and in two components
    ((12.5, 30, 12.5), (0, -1, 0), 100, ((12, 13, 12), 3, 16.0)),
    ((12.5, 12.5, -3), (0, 0, 2), 100, ((12, 12, 10), 4, 6.5)),
    ((8.5, 30, 12.5), (0, -1, 0), 100, None),  # through the box beside the body
    ((6.5, 30, 12.5), (0, -1, 0), 100, None),  # beside the box: d = 0 on an axis whose o lies outside
    # origins on each face of the box, on an edge of it, and inside a body voxel
    ((7, 12.5, 12.5), (1, 0, 0), 100, ((10, 12, 12), 0, 3.0)),
    ((17, 12.5, 12.5), (-1, 0, 0), 100, ((13, 12, 12), 1, 3.0)),
    ((12.5, 7, 12.5), (0, 1, 0), 100, ((12, 10, 12), 2, 3.0)),
    ((12.5, 17, 12.5), (0, -1, 0), 100, ((12, 13, 12), 3, 3.0)),
    ((12.5, 12.5, 7), (0, 0, 1), 100, ((12, 12, 10), 4, 3.0)),
    ((12.5, 12.5, 17), (0, 0, -1), 100, ((12, 12, 13), 5, 3.0)),
    ((7, 7, 12.5), (1, 1, 0), 100, ((10, 10, 12), 2, 3.0)),
    ((17, 12.5, 12.5), (1, 0, 0), 5, None),  # on the far face, leaving: the slab is closed, the voxels are not
    ((11.5, 11.25, 11.75), (0.3, -0.2, 0.9), 100, ((11, 11, 11), 6, 0.0)),
    ((10, 10, 10), (-1, -1, -1), 100, ((10, 10, 10), 6, 0.0)),
    # maxT an ulp below, at and an ulp above the hit's t; +inf
    ((5, 12.5, 12.5), (1, 0, 0), below(5), None),
    ((5, 12.5, 12.5), (1, 0, 0), 5, ((10, 12, 12), 0, 5.0)),
    ((5, 12.5, 12.5), (1, 0, 0), above(5), ((10, 12, 12), 0, 5.0)),
    ((5, 12.5, 12.5), (1, 0, 0), INF, ((10, 12, 12), 0, 5.0)),
    ((5, 12.5, 12.5), (-1, 0, 0), INF, None),
    ((5, 12.5, 12.5), (1, 0, 0), 0, None),
    ((11.5, 11.5, 11.5), (1, 0, 0), 0, ((11, 11, 11), 6, 0.0)),
    # a zero direction tests the origin's voxel alone
    ((11.5, 11.5, 11.5), (0, 0, 0), 100, ((11, 11, 11), 6, 0.0)),
    ((8.5, 8.5, 8.5), (0, 0, 0), 100, None),
    ((1, 1, 1), (0, 0, 0), INF, None),
    # NaN and inf components, a negative and a NaN maxT
    ((NAN, 12.5, 12.5), (1, 0, 0), 100, None),
    ((5, 12.5, 12.5), (1, NAN, 0), 100, None),
    ((INF, 12.5, 12.5), (-1, 0, 0), 100, None),
    ((5, 12.5, 12.5), (INF, 0, 0), 100, None),
    ((5, 12.5, 12.5), (1, 0, -INF), 100, None),
    ((3e30, 12.5, 12.5), (-1, 0, 0), INF, None),
    ((5, 12.5, 12.5), (1, 0, 0), -1, None),
    ((11.5, 11.5, 11.5), (1, 0, 0), -0.0, ((11, 11, 11), 6, 0.0)),  # (-0 is not negative)
    ((5, 12.5, 12.5), (1, 0, 0), NAN, None),
]


def adversarial_scene():
    """(models, instances, rays): the rays above against the wide cube, a tilted copy of scene()'s first model across it, and the cube again."""
    models, instances = wide_cube()
    rng = np.random.default_rng(5)
    models = models + [random_model(rng, (12, 9, 7), zeros=0.4)]
    instances = instances + [gpu.model_instance(forward_about_centre(tilt(), (12, 9, 7), (40, 12, 12)), (12, 9, 7), 1, FILL)]
    return models, instances, rays_of([a[0] for a in ADVERSARIAL], [a[1] for a in ADVERSARIAL], [a[2] for a in ADVERSARIAL])


def assert_adversarial(hits):
    for i, (origin, direction, max_t, want) in enumerate(ADVERSARIAL):
        h, what = hits[i], f"ray {i}: {origin} {direction} maxT {max_t}"
        if want is None:
            assert h["voxel"].tolist() == [-1, -1, -1] and h["face"] == -1 and h["argb"] == 0 and h["instance"] == -1 and h["modelVoxel"].tolist() == [-1, -1, -1], what
            assert h["t"].tobytes() == np.float32(max_t).tobytes(), what  # (maxT as given, a NaN's bits too)
        else:
            voxel, face, t = want
            assert h["voxel"].tolist() == list(voxel) and h["face"] == face and h["instance"] == 0, (what, h)
            assert h["t"].tobytes() == np.float32(t).tobytes(), (what, h)  # (a zero is +0)
            assert h["modelVoxel"].tolist() == [v - 10 for v in voxel] and h["argb"] == cube_model()[0][tuple(np.array(voxel)[[0, 2, 1]] - 10)], what
        assert h["pad_"].tolist() == [0, 0]


STEP_LENGTHS, STEP_LAYERS = (1, 63, 64, 65, 129, 200), (0, 62, 63, 64, 65, 127, 128)


def steps_scene(axis, sign):
    """(models, instances, rays, the voxels): per (box length L along `axis`, layer l < L) a one-voxel body in layer l of the walk -- counted from
    where a ray travelling `sign` along `axis` enters -- of a box L long and 3 x 3 across, and the ray from 2.5 voxels before the box through the
    voxel's centre, off the axis so that it crosses minor planes on the way.  Last: the voxel in layer 64 of a 129-box and a maxT that ends the
    ray in layer 63."""
    rng = np.random.default_rng(100 + 2 * axis + (sign > 0))
    b, c = [a for a in range(3) if a != axis]
    models = [(np.full((1, 1, 1), 0xFF112233, dtype=np.uint32), None)]
    instances, origins, directions, max_t, voxels = [], [], [], [], []
    cases = [(L, l, False) for L in STEP_LENGTHS for l in STEP_LAYERS if l < L] + [(129, 64, True)]
    for n, (L, l, cut) in enumerate(cases):
        lo = [0, 0, 0]
        lo[axis], lo[b], lo[c] = -37 if n % 2 else 11, 10 * n, -5
        hi = list(lo)
        hi[axis], hi[b], hi[c] = lo[axis] + L, lo[b] + 3, lo[c] + 3
        voxel = list(lo)
        voxel[axis], voxel[b], voxel[c] = (lo[axis] + l if sign > 0 else hi[axis] - 1 - l), lo[b] + 1, lo[c] + 1
        instances.append(make_instance(np.eye(3, dtype=np.int64) * ONE, [-v * ONE for v in voxel], lo, hi, 0, FILL))
        start = [0.0, 0.0, 0.0]
        start[axis] = lo[axis] - 2.5 if sign > 0 else hi[axis] + 2.5
        start[b], start[c] = lo[b] + rng.uniform(0.2, 2.8), lo[c] + rng.uniform(0.2, 2.8)
        d = np.array(voxel) + 0.5 - np.array(start)
        d /= abs(d[axis])
        origins.append(start)
        directions.append(d)
        max_t.append(2.5 + l - 0.5 if cut else 1e4)  # (the voxel's layer begins at t = 2.5 + l)
        voxels.append(None if cut else voxel)
    return models, instances, rays_of(origins, directions, max_t), voxels


def assert_steps(scene, hits):
    models, instances, rays, voxels = scene
    for i, voxel in enumerate(voxels):
        if voxel is None:
            assert hits[i]["instance"] == -1 and hits[i]["face"] == -1, f"ray {i} ends a layer before its voxel"
        else:
            assert hits[i]["voxel"].tolist() == voxel and hits[i]["instance"] == i and hits[i]["modelVoxel"].tolist() == [0, 0, 0] and hits[i]["argb"] == 0xFF112233, (i, hits[i])


def line_scene(order=(0, 1, 2, 3, 4), twice=False):
    """Five cubes in a line along x, listed in `order` (twice: every one listed twice, one behind the other in the list); rays along the line
    from both ends and across it onto every cube."""
    at = [(10 * k, 0, 0) for k in range(5)]
    instances = [identity_at(at[k], CUBE, 0, FILL) for k in order for _ in range(2 if twice else 1)]
    origins = [(-5, 1.5, 2.5), (60, 2.5, 1.5)] + [(10 * k + 1.5, 20, 2.5) for k in range(5)] + [(10 * k + 2.5, 1.5, -9) for k in range(5)] + [(22, 9, 2)]
    directions = [(1, 0, 0), (-1, 0, 0)] + [(0, -1, 0)] * 5 + [(0, 0, 1)] * 5 + [(1, 0, 0)]
    return [cube_model()], instances, rays_of(origins, directions, 1e4)


LINE_BODIES = [0, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, -1]  # the cube each ray of line_scene hits


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------

def test_the_scene_covers_what_it_should():
    models, instances, rays, (want, amb) = scene()
    boxes = np.array([[list(i.boxMin), list(i.boxMax)] for i in instances])
    assert boxes[:, 0, 1].min() < 0 and boxes[:, 0, 0].min() < 0, "a box below y = 0 and one below x = 0"
    overlaps = sum(1 for a in range(8) for b in range(a) if (np.maximum(boxes[a, 0], boxes[b, 0]) < np.minimum(boxes[a, 1], boxes[b, 1])).all())
    assert overlaps >= 3
    assert 1 - amb.mean() >= 0.99
    assert 0.25 <= (want["instance"] >= 0).mean() <= 0.75 and set(want["instance"].tolist()) == set(range(-1, 8))
    assert set(want["face"].tolist()) >= set(range(-1, 7))


def test_rules_match_the_model_on_the_scene(rules, tmp_path):
    models, instances, rays, model = scene()
    hits, jobs = run_cases(rules, tmp_path, [(models, instances, rays)])[0]
    assert jobs > len(rays)
    assert modelpickmodel.compare(hits, model, "scene") >= 0.99
    assert (hits["pad_"] == 0).all() and (hits["t"][hits["instance"] < 0] == rays["maxT"][hits["instance"] < 0]).all()


def test_adversarial_rays_by_hand(rules, tmp_path):
    hits, _ = run_cases(rules, tmp_path, [adversarial_scene()])[0]
    assert_adversarial(hits)


def grid_rays(n=3000):
    """Rays made of ties: origins on the half-voxel grid around scene()'s bodies, direction components from a few powers of two and 0, so that
    crossings of two and three axes coincide all along the way; a few from far away and with tiny components, where the products round."""
    rng = np.random.default_rng(77)
    o = np.stack([rng.integers(0, 120, size=n), rng.integers(-10, 70, size=n), rng.integers(20, 120, size=n)], axis=-1) * 0.5
    d = rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=(n, 3))
    far = np.arange(n) % 10 == 0
    d[far] = d[far] + rng.choice([0.0, 1e-30, -3e-7], size=(int(far.sum()), 3))
    o[far] = o[far] - d[far] * rng.choice([0.0, 3e4, 1e7], size=(int(far.sum()), 1))
    return rays_of(o, d, np.where(np.arange(n) % 7 == 0, rng.integers(1, 40, size=n) * 0.5, 1e9))


def test_layers_equal_the_rule_where_crossings_coincide(rules, tmp_path):
    """(The program compares every job of the two forms.)  The rays are nearly all ambiguous to any other rule: nothing else is compared."""
    models, instances, _, _ = scene()
    hits, jobs = run_cases(rules, tmp_path, [(models, instances, grid_rays())])[0]
    assert jobs > 2000 and (hits["instance"] >= 0).mean() > 0.1 and (hits["face"] == 6).any()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_the_steps_of_the_walk(rules, tmp_path, axis, sign):
    s = steps_scene(axis, sign)
    hits, _ = run_cases(rules, tmp_path, [s[:3]])[0]
    assert_steps(s, hits)
    model = modelpickmodel.pick_many(s[0], as_dicts(s[1]), s[2]["origin"], s[2]["direction"], s[2]["maxT"])
    modelpickmodel.compare(hits, model, f"steps {axis} {sign}")


def test_the_ray_rule(rules, tmp_path):
    order = (3, 0, 4, 2, 1)
    (plain, _), (permuted, _), (twice, _) = run_cases(rules, tmp_path, [line_scene(), line_scene(order), line_scene(twice=True)])
    assert plain["instance"].tolist() == LINE_BODIES
    assert plain["t"][:2].tolist() == [5.0, 16.0] and plain["face"][:2].tolist() == [0, 1]
    assert permuted["instance"].tolist() == [order.index(k) if k >= 0 else -1 for k in LINE_BODIES]
    for name in ("voxel", "face", "argb", "t", "modelVoxel", "pad_"):
        assert permuted[name].tobytes() == plain[name].tobytes(), name
    assert twice["instance"].tolist() == [2 * k if k >= 0 else -1 for k in LINE_BODIES], "of two identical instances the lower index wins"
    for name in ("voxel", "face", "argb", "t", "modelVoxel"):
        assert twice[name].tobytes() == plain[name].tobytes(), name


MESSAGES = [
    "models NULL or modelCount 1 outside 1 .. 256", "models NULL or modelCount 257 outside 1 .. 256", "instances NULL or instanceCount 2 outside 1 .. 4096",
    "instances NULL or instanceCount 4097 outside 1 .. 4096", "model 0: size 0 on axis 1 is below 1", "model 0: argb and solid are both NULL",
    "instance 1: model 1 outside 0 .. 0", "instance 1: the box [0, 0) on axis 1 is empty", "instance 0: the box [0, 1073741825) on axis 2 has a coordinate beyond 2^30",
    "instance 1: toModel: m[1][2] = 16777217 beyond 2^24 (256 in units of 2^-16)", "instance 1: toModel: t[2] = -70368744177665 beyond 2^46 (2^30 in units of 2^-16)",
    "rays is NULL", "hits is NULL", "rayCount 0 outside 1 .. 65536", "rayCount -1 outside 1 .. 65536", "rayCount 65537 outside 1 .. 65536",
]


def _check_args(text):
    lines = text.splitlines()
    assert lines[:2] == ["-1", "-1"], "without a context"
    at = 2
    for message in MESSAGES:
        assert lines[at] == f"-1 cvxq_model_pick: {message}" and lines[at + 1] == f"-1 cvxq_model_pick_device: {message}", (lines[at], message)
        at += 2
    assert at == len(lines)


def test_calls_fail_cleanly_with_their_messages(rules):
    """(The program itself fails when an error wrote to the host array.)"""
    _check_args(subprocess.check_output([rules, "args"], text=True))


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    inst = [identity_at((0, 0, 0), (2, 2, 2))]
    with pytest.raises(ValueError, match="model_pick: a model is a pair"):
        ctx.model_pick([np.zeros((2, 2, 2), dtype=np.uint32)], inst, [(0, 0, 0)], [(1, 0, 0)], 1.0)
    with pytest.raises(ValueError, match="model_pick: one direction per origin"):
        ctx.model_pick([(np.zeros((2, 2, 2), dtype=np.uint32), None)], inst, [(0, 0, 0)], [(1, 0, 0), (0, 1, 0)], 1.0)
    with pytest.raises(ValueError, match="model_pick_device: a model is"):
        ctx.model_pick_device([(1, 2)], inst, None, None)
    assert gpu.MODEL_HIT_DTYPE.itemsize == 48 and gpu.MODEL_PICK_MAX_RAYS == 65536


def test_the_rules_run_clean_under_the_sanitizers(rules, tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python) built with -fsanitize=address,undefined: the argument checks,
    the adversarial rays, the ray rule and one set of steps run to the end and give the bytes of the plain build."""
    program = ruleslib.build("model_pick_rules", tmp_path, *SANITIZE)
    _check_args(subprocess.check_output([program, "args"], text=True))
    cases = [adversarial_scene(), line_scene(twice=True), steps_scene(1, -1)[:3]]
    plain, clean = tmp_path / "plain", tmp_path / "clean"
    plain.mkdir()
    clean.mkdir()
    for (a, ja), (b, jb) in zip(run_cases(rules, plain, cases), run_cases(program, clean, cases)):
        assert a.tobytes() == b.tobytes() and ja == jb
