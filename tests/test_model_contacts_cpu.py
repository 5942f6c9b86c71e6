"""CPU (no GPU needed): the rules behind cvxp_model_contacts / cvxp_box_pairs / cvxp_pair_response (cpuvox_amd/csrc/cvx_pair_contacts.h), compiled
for the host through tests/pair_contacts_rules.cpp, against the independent numpy model of tests/paircontactsmodel.py.  The program runs the
scalar specification (cvxb::PairOf) AND the kernels' walk (a wave per job, 64 lanes a step, the job's sums added as the atomics add them) and fails
when they differ in a byte; its output must equal the model's bytes.  Everything is integers: no comparison has a tolerance.

- The scenes of the GPU test (tests/test_gpu_model_contacts.py builds them here): the two cubes with their numbers by hand, the mixed call, the
  steps of the walk, bodies clipped by their own boxes, pairs with empty intersections, the lattice of more than 1024 pairs; what each has to
  cover is asserted from the model first.
- Random small calls (seed 20261) under rotations, a mirror, scale 2 and 1/2, with boxes hundreds of voxels taller than their bodies and boxes
  tighter than them.
- Every argument check with its message, cvxp_box_pairs against the double loop, cvxp_pair_response against the formula in Python float64, the
  wrappers' array checks.
- The same stand-alone program built with -fsanitize=address,undefined (the header's mirrors: tests/test_abi_pair_contacts.py)."""
import subprocess

import numpy as np
import pytest

import paircontactsmodel
import ruleslib
from cpuvox_amd import gpu
from test_world_contacts_cpu import CUBE, MAPS, SANITIZE, cube_model
from test_world_models_cpu import as_dicts, call_words, forward_about_centre, identity_at, mixed_call, random_model, rotation, tilt

FILL = gpu.BRUSH_FILL


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("pair_contacts_rules", tmp_path_factory.mktemp("pair_contacts"))


# ---- building calls (the GPU test uses these too) -----------------------------------------------------------------------------------------------

def model_of(models, instances, pairs):
    return paircontactsmodel.contacts(models, as_dicts(instances), pairs)


def full_model(size, colour=0xFF203040, with_argb=True):
    """A model of `size` (sx, sy, sz) with every voxel set; arrays are (X, Z, Y)."""
    shape = (size[0], size[2], size[1])
    return (np.full(shape, colour, dtype=np.uint32), None) if with_argb else (None, np.ones(shape, dtype=bool))


def scene_cubes():
    """Two 4 x 4 x 4 identity cubes, a (index 0) sunk one layer into b (index 1) from above; the pair and its reverse."""
    return [cube_model()], [identity_at((10, 13, 10), CUBE, 0, FILL), identity_at((10, 10, 10), CUBE, 0, FILL)], np.int32([[0, 1], [1, 0]])


def scene_mixed():
    """tests/test_world_models_cpu.py's mixed call packed into a 26 x 64 x 26 space so that the bodies meet, one more instance of a mask-only model,
    the pairs box_pairs finds, the first touching one of them listed again, and the second reversed."""
    rng = np.random.default_rng(12)
    _, models, instances = mixed_call(rng, (26, 64, 26), FILL)
    mask = random_model(rng, (7, 9, 8), with_mask=True, zeros=0.2)[1]
    models = models + [(None, mask)]
    instances = instances + [gpu.model_instance(forward_about_centre(rotation(2, 25), (7, 9, 8), (14, 9, 13)), (7, 9, 8), len(models) - 1, FILL)]
    found = paircontactsmodel.box_pairs(as_dicts(instances))
    touching = np.nonzero(paircontactsmodel.contacts(models, as_dicts(instances), found)[0]["overlap"] > 0)[0]
    pairs = np.concatenate([found, found[touching[:1]], found[touching[1:2], ::-1]])
    return models, instances, pairs


def scene_steps():
    """The steps of the walk.  Pair 0: two 5 x 100 x 5 bodies, X_p 100 tall: the first step ends at y = 36 (lane 63), the second begins at 35
    (lane 0).  Pair 1 and 2: boxes 500 and more tall around a cube and a tilted body (the cut).  Pair 3: a 3 x 64 x 3 body whose box and image
    end at y = 0, the last lane of X_p's one step, in a body that goes on below."""
    rng = np.random.default_rng(4)
    models = [random_model(rng, (5, 100, 5), zeros=0.25), random_model(rng, (5, 100, 5), with_mask=True, zeros=0.25), cube_model(), random_model(rng, (5, 6, 4), zeros=0.2),
              full_model((3, 64, 3)), full_model((3, 130, 3), with_argb=False)]
    instances = [identity_at((0, 0, 0), (5, 100, 5), 0, FILL), identity_at((1, 0, 1), (5, 100, 5), 1, FILL)]
    tall = [identity_at((20, 7, 20), CUBE, 2, FILL), gpu.model_instance(forward_about_centre(tilt(), (5, 6, 4), (22, 9, 22)), (5, 6, 4), 3, FILL),
            gpu.model_instance(forward_about_centre(rotation(0, 90), (5, 100, 5), (21, 8, 21)), (5, 100, 5), 0, FILL)]
    for k, inst in enumerate(tall):
        inst.boxMin[1] -= 300 + 7 * k
        inst.boxMax[1] += 200 + 64 * k
    instances += tall
    instances += [identity_at((40, 0, 40), (3, 64, 3), 4, FILL), identity_at((40, -2, 40), (3, 130, 3), 5, FILL)]
    return models, instances, np.int32([[0, 1], [2, 3], [4, 3], [5, 6], [2, 4]])


def scene_clipped():
    """Bodies clipped by their own boxes: 6 x 6 x 6 full cubes whose instance boxes are a voxel tighter than their images on every side, and a yaw
    of 45 degrees clipped the same way."""
    models = [full_model((6, 6, 6)), full_model((6, 6, 6), 0xFF0A0B0C)]
    a, b = identity_at((0, 0, 0), (6, 6, 6), 0, FILL), identity_at((2, 2, 2), (6, 6, 6), 1, FILL)
    c = gpu.model_instance(forward_about_centre(rotation(1, 45), (6, 6, 6), (4, 4, 4)), (6, 6, 6), 0, FILL)
    for inst in (a, b, c):
        for i in range(3):
            inst.boxMin[i] += 1 if inst is not c else 3
            inst.boxMax[i] -= 1 if inst is not c else 3
    return models, [a, b, c], np.int32([[0, 1], [1, 0], [0, 2], [2, 1]])


def scene_empty(only=False):
    """Cubes of which 0, 1 and 2 meet in a corner and 3 and 4 lie far away (4 in another octant): pairs with an empty X_p first, in the middle and last
    among touching ones, or (only=True) alone."""
    instances = [identity_at(at, CUBE, 0, FILL) for at in ((0, 0, 0), (3, 1, 2), (3, 2, 1), (100, 0, 0), (-50, -60, 7))]
    if only:
        return [cube_model()], instances, np.int32([[0, 3], [4, 1], [3, 4]])
    return [cube_model()], instances, np.int32([[0, 3], [4, 2], [0, 1], [1, 3], [3, 4], [2, 1], [0, 2], [2, 4], [3, 0]])


def scene_lattice(n=6):
    """n^3 cubes of 3 x 3 x 3 spaced two apart: neighbours share a layer, a line or a voxel.  6^3 cubes make 1940 pairs."""
    model = random_model(np.random.default_rng(8), (3, 3, 3), zeros=0.1)
    instances = [identity_at((2 * x, 2 * y, 2 * z), (3, 3, 3), 0, FILL) for x in range(n) for y in range(n) for z in range(n)]
    return [model], instances, paircontactsmodel.box_pairs(as_dicts(instances))


def clipped_neighbours(models, instances, pairs):
    """Per axis, how many overlap voxels of the pairs have a neighbour that body a's MAP calls set but a's box excludes (from the model alone)."""
    counts = np.zeros(3, dtype=int)
    dicts = as_dicts(instances)
    for a, b in pairs:
        ia, ib = dicts[a], dicts[b]
        lo = [max(ia["box_min"][i], ib["box_min"][i]) for i in range(3)]
        hi = [min(ia["box_max"][i], ib["box_max"][i]) for i in range(3)]
        if any(lo[i] >= hi[i] for i in range(3)):
            continue
        wide = dict(ia, box_min=[v - 2 for v in ia["box_min"]], box_max=[v + 2 for v in ia["box_max"]])  # the map without the box
        wlo, whi = [v - 1 for v in lo], [v + 1 for v in hi]
        real, mapped = paircontactsmodel.body_in(models, ia, wlo, whi), paircontactsmodel.body_in(models, wide, wlo, whi)
        o = real[1:-1, 1:-1, 1:-1] & paircontactsmodel.body_in(models, ib, lo, hi)
        for axis in range(3):
            for step in (-1, 1):
                shifted = [slice(1, -1)] * 3
                shifted[axis] = slice(1 + step, real.shape[axis] - 1 + step)
                counts[axis] += int((o & mapped[tuple(shifted)] & ~real[tuple(shifted)]).sum())
    return counts


def pair_words(models, instances, pairs):
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return [call_words(models, instances), [len(pairs)], pairs.ravel()]


def parse(raw, counts):
    """The bytes pair_contacts_rules writes for cases of `counts` pairs -> [(results, points, summary dict)]."""
    out, at = [], 0
    for n in counts:
        results = np.frombuffer(raw[at:at + 144 * n], dtype=paircontactsmodel.RESULT_DTYPE)
        at += 144 * n
        summary = dict(zip(paircontactsmodel.SUMMARY_NAMES, (int(v) for v in np.frombuffer(raw[at:at + 32], dtype=np.int64))))
        at += 32
        points = np.frombuffer(raw[at:at + 32 * summary["points"]], dtype=paircontactsmodel.POINT_DTYPE)
        at += 32 * summary["points"]
        out.append((results, points, summary))
    assert at == len(raw)
    return out


def same(got, want, what=""):
    """Results, points and summary byte for byte."""
    (r, p, s), (mr, mp, ms) = got, want
    for name in paircontactsmodel.RESULT_DTYPE.names:
        assert (np.asarray(r[name]) == mr[name]).all(), f"{what}: results differ in `{name}`: {r[name].tolist()} vs the model's {mr[name].tolist()}"
    assert r.tobytes() == mr.tobytes(), what
    assert s == ms, f"{what}: summary {s} vs the model's {ms}"
    for name in paircontactsmodel.POINT_DTYPE.names:
        assert len(p) == len(mp) and (np.asarray(p[name]) == mp[name]).all(), f"{what}: the points differ in `{name}`"
    assert p.tobytes() == mp.tobytes(), f"{what}: the points differ"


def run_cases(rules, tmp_path, cases):
    """cases: [(models, instances, pairs)] -> the program's parsed output."""
    parts = []
    for case in cases:
        parts += pair_words(*case)
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *parts, dtype=np.uint8).tobytes()
    return parse(raw, [len(case[2]) for case in cases])


def check_against_model(rules, tmp_path, cases, what=""):
    got = run_cases(rules, tmp_path, cases)
    want = [model_of(*c) for c in cases]
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"{what} case {k}")
    return want


def assert_cubes(results, points, summary):
    """The numbers of scene_cubes by hand: the shared layer y = 13 is 16 voxels; b's open faces there sum to 16 e_y (the side faces of the
    layer's rim cancel), a's to -16 e_y."""
    r = results[0]
    assert (r["overlap"], r["points"], r["firstPoint"], r["a"], r["b"], r["pad_"]) == (16, 16, 0, 0, 1, 0)
    assert r["pushA"].tolist() == [0, 16, 0] and r["pushB"].tolist() == [0, -16, 0]
    assert r["origin"].tolist() == [10, 13, 10] and r["sum"].tolist() == [24, 0, 24] and r["min"].tolist() == [10, 13, 10] and r["max"].tolist() == [14, 14, 14]
    for which, normal in ((0, [0.0, 1.0, 0.0]), (1, [0.0, -1.0, 0.0])):
        centre, n, depth = gpu.pair_response(r, which)
        assert depth == 1.0 and n.tolist() == normal and centre.tolist() == [12.0, 13.5, 12.0]
    back = results[1]
    assert (back["a"], back["b"], back["firstPoint"]) == (1, 0, 16), "the reversed pair"
    assert back["pushA"].tolist() == r["pushB"].tolist() and back["pushB"].tolist() == r["pushA"].tolist() and back["overlap"] == 16
    for name in ("sum", "origin", "min", "max"):
        assert back[name].tolist() == r[name].tolist()
    first, second = points[points["pair"] == 0], points[points["pair"] == 1]
    assert len(first) == len(second) == 16 and (first["voxel"] == second["voxel"]).all() and (first["voxel"][:, 1] == 13).all()
    assert (first["facesA"] == second["facesB"]).all() and (first["facesB"] == second["facesA"]).all() and (first["argbA"] == 0xFF112233).all()
    assert (first["facesA"] & 0x04).all() and (first["facesB"] & 0x08).all() and not (first["facesA"] & 0x08).any()
    assert first["voxel"][:, [0, 2]].tolist() == [[x, z] for x in range(10, 14) for z in range(10, 14)]
    assert summary == dict(touching=2, overlap=32, points=32, jobs=32)


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------------------

def test_two_cubes_by_hand(rules, tmp_path):
    want = check_against_model(rules, tmp_path, [scene_cubes()], "cubes")[0]
    assert_cubes(*want)


def assert_mixed(scene, want):
    models, instances, pairs = scene
    results = want[0]
    assert (results["overlap"] > 0).sum() >= 4 and want[2]["points"] > 100
    used = {instances[k].model for k in pairs[results["overlap"] > 0].ravel()}
    assert any(models[m][0] is None for m in used) and any(models[m][0] is not None and models[m][1] is not None for m in used), "mask-only, and both arrays"
    twin = int(np.nonzero((pairs[:-2] == pairs[-2]).all(axis=1))[0][0])
    assert results[-2]["overlap"] == results[twin]["overlap"] > 0 and results[-2]["firstPoint"] > results[twin]["firstPoint"], "a pair listed twice"
    assert results[-1]["overlap"] > 0 and (pairs[:-2] == pairs[-1][::-1]).all(axis=1).any(), "and one reversed"
    assert (results["pushA"] != 0).any(axis=1).sum() >= 3 and ((results["pushA"] != 0).sum(axis=1) >= 2).any()


def test_the_mixed_call(rules, tmp_path):
    scene = scene_mixed()
    want = check_against_model(rules, tmp_path, [scene], "mixed")[0]
    assert_mixed(scene, want)


def assert_steps(scene, want):
    models, instances, pairs = scene
    results, points, _ = want
    d = as_dicts(instances)
    o = paircontactsmodel.body_in(models, d[0], (1, 0, 1), (5, 100, 5)) & paircontactsmodel.body_in(models, d[1], (1, 0, 1), (5, 100, 5))
    assert (o[:, 36, :] & o[:, 35, :]).any() and (o[:, 36, :] & ~o[:, 35, :]).any() and (~o[:, 36, :] & o[:, 35, :]).any(), "overlap on both sides of the step boundary"
    for p in (1, 2, 4):
        a, b = pairs[p]
        assert min(d[a]["box_max"][1], d[b]["box_max"][1]) - max(d[a]["box_min"][1], d[b]["box_min"][1]) > 256 + 64 and results[p]["overlap"] > 0, "the cut"
    assert results[2]["points"] > 0 and results[4]["points"] > 0
    r = results[3]
    assert (r["origin"][1], r["min"][1], r["max"][1], r["overlap"]) == (0, 0, 64, 9 * 64), "ends at the step's last lane"
    last = points[(points["pair"] == 3) & (points["voxel"][:, 1] == 0)]
    assert len(last) == 9 and (last["facesA"] & 0x04).all() and not (last["facesB"] & 0x04).any(), "below y = 0 lies b alone"


def test_the_steps_of_the_walk(rules, tmp_path):
    scene = scene_steps()
    assert_steps(scene, check_against_model(rules, tmp_path, [scene], "steps")[0])


def assert_clipped(scene, want):
    models, instances, pairs = scene
    assert (clipped_neighbours(models, instances, pairs[:1]) > 0).all() and (clipped_neighbours(models, instances, pairs[2:3]) > 0).all(), "on x, on y and on z"
    r = want[0][0]  # boxes [1, 5)^3 and [3, 7)^3: O = [3, 5)^3, every outward face open in one of the two
    assert r["overlap"] == 8 and r["points"] == 8 and r["pushB"].tolist() == [4, 4, 4] and r["pushA"].tolist() == [-4, -4, -4]
    assert set(want[1]["facesA"][want[1]["pair"] == 0].tolist()) == {0x2A, 0x28, 0x22, 0x0A, 0x20, 0x08, 0x02, 0x00}


def test_bodies_clipped_by_their_own_boxes(rules, tmp_path):
    scene = scene_clipped()
    assert_clipped(scene, check_against_model(rules, tmp_path, [scene], "clipped")[0])


def assert_empty(scene, want, only):
    results, _, summary = want
    empty = np.array([a in (3, 4) or b in (3, 4) for a, b in scene[2]])
    assert (results["overlap"][empty] == 0).all() and not results["max"][empty].any() and empty[0] and empty[-1] and empty[1:-1].any()
    if only:
        assert empty.all() and summary == dict(touching=0, overlap=0, points=0, jobs=0)
        assert results["origin"].tolist() == [[100, 0, 0], [3, 1, 7], [100, 0, 7]], "the maximum of the two boxMin all the same"
    else:
        assert (results["overlap"][~empty] > 0).all() and summary["touching"] == (~empty).sum() == 3 and not empty[2] and not empty[5]


@pytest.mark.parametrize("only", [False, True])
def test_pairs_with_empty_intersections(rules, tmp_path, only):
    scene = scene_empty(only)
    assert_empty(scene, check_against_model(rules, tmp_path, [scene], "empty")[0], only)


def test_the_lattice(rules, tmp_path):
    scene = scene_lattice()
    assert len(scene[2]) == 1940 > 1024
    want = check_against_model(rules, tmp_path, [scene], "lattice")[0]
    assert want[2]["touching"] > 1024 and len(set(want[0]["overlap"].tolist())) >= 3


# ---- random small calls -------------------------------------------------------------------------------------------------------------------------

def random_calls():
    """The 160 random calls (seed 20261) as [(models, instances, pairs, the name of every instance's map)]; the GPU tests run them too."""
    rng = np.random.default_rng(20261)
    names = sorted(MAPS)
    cases = []
    for n in range(160):
        models = [random_model(rng, (3, 5, 4), with_mask=bool(n % 2), zeros=0.2), random_model(rng, (2, 70, 2), zeros=0.1)]
        if n % 3 == 0:
            models[0] = (None, models[0][1] if models[0][1] is not None else models[0][0] != 0)  # a model without argb
        instances, used = [], []
        for _ in range(int(rng.integers(2, 5))):
            model = int(rng.integers(0, 2))
            name = names[int(rng.integers(0, len(names)))]
            size = (3, 5, 4) if model == 0 else (2, 70, 2)
            inst = gpu.model_instance(forward_about_centre(MAPS[name], size, tuple(rng.uniform(-3, 3, 3))), size, model, int(rng.integers(0, 4)))
            draw = rng.random()
            if draw < 0.3:  # a box far taller than the body
                inst.boxMin[1] -= int(rng.integers(0, 400))
                inst.boxMax[1] += int(rng.integers(100, 400))
            elif draw < 0.6:  # a box tighter than the body
                for i in range(3):
                    if inst.boxMax[i] - inst.boxMin[i] > 4:
                        inst.boxMin[i] += int(rng.integers(0, 3))
                        inst.boxMax[i] -= int(rng.integers(0, 3))
            instances.append(inst)
            used.append(name)
        k = len(instances)
        pairs = np.int32([(a, b) for a in range(k) for b in range(k) if a != b])
        pairs = pairs[rng.permutation(len(pairs))[:int(rng.integers(1, len(pairs) + 1))]]
        cases.append((models, instances, pairs, used))
    return cases


def test_both_forms_match_the_model_on_random_calls(rules, tmp_path):
    names = sorted(MAPS)
    cases = random_calls()
    want = [model_of(*c[:3]) for c in cases]
    touching = {name: 0 for name in names}
    tall = clipped = empty = with_points = buried = 0
    for (models, instances, pairs, used), (results, points, summary) in zip(cases, want):
        d = as_dicts(instances)
        for (a, b), r in zip(pairs, results):
            height = min(d[a]["box_max"][1], d[b]["box_max"][1]) - max(d[a]["box_min"][1], d[b]["box_min"][1])
            tall += height > 256 and r["overlap"] > 0
            empty += any(max(d[a]["box_min"][i], d[b]["box_min"][i]) >= min(d[a]["box_max"][i], d[b]["box_max"][i]) for i in range(3))
            touching[used[a]] += r["overlap"] > 0
            buried += r["overlap"] > r["points"] > 0
        with_points += summary["points"] > 0
        clipped += (clipped_neighbours(models, instances, pairs) > 0).any()
    assert all(v > 5 for v in touching.values()), touching
    assert tall > 10 and clipped > 10 and empty > 3 and with_points > 80 and buried > 5, (tall, clipped, empty, with_points, buried)
    got = run_cases(rules, tmp_path, [c[:3] for c in cases])
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"case {k}")


# ---- arguments, the helpers, the wrappers -------------------------------------------------------------------------------------------------------

MESSAGES = [
    "models NULL or modelCount 1 outside 1 .. 256", "models NULL or modelCount 257 outside 1 .. 256", "instances NULL or instanceCount 2 outside 1 .. 4096",
    "instances NULL or instanceCount 4097 outside 1 .. 4096", "model 0: size 0 on axis 1 is below 1", "model 0: argb and solid are both NULL",
    "instance 1: model 1 outside 0 .. 0", "instance 1: the box [0, 0) on axis 1 is empty", "instance 0: the box [0, 1073741825) on axis 2 has a coordinate beyond 2^30",
    "instance 1: toModel: m[1][2] = 16777217 beyond 2^24 (256 in units of 2^-16)", "instance 1: toModel: t[2] = -70368744177665 beyond 2^46 (2^30 in units of 2^-16)",
    "pairs NULL or pairCount 1 outside 1 .. 65536", "pairs NULL or pairCount 0 outside 1 .. 65536", "pairs NULL or pairCount 65537 outside 1 .. 65536",
    "pair 2: (1, 2) has an index outside 0 .. 1", "pair 0: (-1, 0) has an index outside 0 .. 1", "pair 1: (1, 1) pairs an instance with itself",
    "results is NULL", "pointCapacity -1 with a list", "pointCapacity 2 with no list",
]


def _check_args(text):
    lines = text.splitlines()
    assert lines[:2] == ["-1", "-1"], "without a context"
    at = 2
    for message in MESSAGES:
        assert lines[at] == f"-1 cvxp_model_contacts: {message}" and lines[at + 1] == f"-1 cvxp_model_contacts_device: {message}", (lines[at], message)
        at += 2
    assert lines[at] == "-4 cvxp_model_contacts: the pairs' common footprints sum to 2^31 - 1 or more (pair, column) jobs"
    assert lines[at + 1] == "-4 cvxp_model_contacts_device: the pairs' common footprints sum to 2^31 - 1 or more (pair, column) jobs"
    assert [line.strip() for line in lines[at + 2:at + 11]] == ["-1"] * 7 + ["0 1", "0 0"], "cvxp_box_pairs"
    assert [line.strip() for line in lines[at + 11:]] == ["-1"] * 5 + ["0", "0"], "cvxp_pair_response"


def test_calls_fail_cleanly_with_their_messages(rules):
    """(The program itself fails when an error wrote to the host arrays.)"""
    _check_args(subprocess.check_output([rules, "args"], text=True))


def _box_pair_cases():
    rng = np.random.default_rng(6)
    cases = []
    touching = [identity_at((0, 0, 0), CUBE), identity_at((4, 0, 0), CUBE), identity_at((0, 4, 0), CUBE), identity_at((3, 3, 3), CUBE), identity_at((9, 9, 9), CUBE)]
    for margin, capacity in ((0, 16), (1, 16), (3, 16), (1, 2), (1, 0)):
        cases.append((touching, margin, capacity))
    for n in range(40):
        count = int(rng.integers(0, 40))
        instances = []
        for _ in range(count):
            at = [int(v) for v in rng.integers(-20, 20, 3)]
            instances.append(identity_at(at, [int(v) for v in rng.integers(1, 9, 3)]))
        cases.append((instances, int(rng.choice([0, 0, 1, 5])), int(rng.choice([0, 3, 2000]))))
    cases.append(([identity_at((-(1 << 30), 0, 0), (2, 2, 2)), identity_at(((1 << 30) - 2, 0, 0), (2, 2, 2))], 1 << 20, 4))  # (no overflow at the limits)
    return cases


def _check_box_pairs(program, tmp_path):
    cases = _box_pair_cases()
    parts = []
    for instances, margin, capacity in cases:
        parts += [[len(instances)]] + [np.frombuffer(bytes(i), dtype=np.int32) for i in instances] + [[margin, capacity]]
    out = ruleslib.run_cases(program, "boxpairs", tmp_path, *parts, dtype=np.int32)
    at, found_more, cut = 0, 0, 0
    for instances, margin, capacity in cases:
        want = paircontactsmodel.box_pairs(as_dicts(instances), margin)
        written = min(len(want), capacity)
        assert out[at] == 0 and out[at + 1] == len(want), (margin, capacity)
        assert out[at + 2:at + 2 + 2 * written].reshape(-1, 2).tolist() == want[:written].tolist()
        at += 2 + 2 * written
        found_more += len(want) > 3
        cut += 0 < capacity < len(want)
    assert at == len(out) and found_more > 10 and cut > 3
    d = as_dicts(cases[0][0])
    assert paircontactsmodel.box_pairs(d, 0).tolist() == [[0, 3], [1, 3], [2, 3]], "boxes that only touch do not intersect"
    assert paircontactsmodel.box_pairs(d, 1).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]] and len(paircontactsmodel.box_pairs(d, 3)) == 10


def test_box_pairs_against_the_double_loop(rules, tmp_path):
    _check_box_pairs(rules, tmp_path)
    instances = _box_pair_cases()[7][0]
    assert gpu.box_pairs(instances, 1).tolist() == paircontactsmodel.box_pairs(as_dicts(instances), 1).tolist() and gpu.box_pairs([]).shape == (0, 2)
    with pytest.raises(ValueError, match="margin"):
        gpu.box_pairs(instances, -1)


def test_pair_response_is_the_formula():
    """The helper's doubles equal the same formula in Python float64, bit for bit, on model results and on large hand-made sums."""
    results = model_of(*scene_mixed())[0]
    results = results[results["overlap"] > 0]
    assert len(results) >= 4
    big = np.zeros(3, dtype=paircontactsmodel.RESULT_DTYPE)
    big["overlap"] = [3, (1 << 53) + 1, 7]
    big["sum"] = [[(1 << 64) - 1, 10, 1 << 63], [12345678901234567, 3, 0], [1, 2, 4]]
    big["pushA"] = [[-(1 << 40), 3, 1 << 62], [1, -1, 1], [0, 0, 0]]
    big["pushB"] = [[5, -7, 11], [1 << 50, 3, 3], [0, 2, 0]]
    big["origin"] = [[-(1 << 30), 1 << 30, 7], [0, -5, 9], [1, 2, 3]]
    for r in list(results) + list(big):
        for which in (0, 1):
            centre, normal, depth = gpu.pair_response(r, which)
            want_centre, want_normal, want_depth = paircontactsmodel.response(r, which)
            assert centre.tobytes() == want_centre.tobytes() and normal.tobytes() == want_normal.tobytes() and np.float64(depth).tobytes() == np.float64(want_depth).tobytes()
    assert gpu.pair_response(big[2], 0)[2] == 0.0 and gpu.pair_response(big[2], 1)[2] == 3.5
    none = np.zeros(1, dtype=paircontactsmodel.RESULT_DTYPE)
    with pytest.raises(ValueError, match="no overlap"):
        gpu.pair_response(none[0], 0)
    with pytest.raises(ValueError, match="which"):
        gpu.pair_response(big[0], 2)


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    inst = [identity_at((0, 0, 0), (2, 2, 2)), identity_at((1, 0, 0), (2, 2, 2))]
    argb = np.zeros((2, 3, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="model_contacts: argb and solid are arrays of one shape"):
        gpu.Context.model_contacts(ctx, [(argb, np.zeros((2, 3, 5), dtype=bool))], inst)
    with pytest.raises(ValueError, match="model_contacts: a model is a pair"):
        gpu.Context.model_contacts(ctx, [argb], inst)
    with pytest.raises(ValueError, match="ModelInstance"):
        gpu.Context.model_contacts(ctx, [(argb, None)], [dict(op=0)])
    with pytest.raises(ValueError, match="model_contacts: pairs is an"):
        gpu.Context.model_contacts(ctx, [(argb, None)], inst, pairs=[0, 1, 2])
    with pytest.raises(ValueError, match="model_contacts_device: a model is"):
        gpu.Context.model_contacts_device(ctx, [((2, 2), 0, 0)], inst, None, None)
    assert gpu.PAIR_RESULT_DTYPE == paircontactsmodel.RESULT_DTYPE and gpu.PAIR_POINT_DTYPE == paircontactsmodel.POINT_DTYPE
    assert gpu.PAIRS_SUMMARY_DTYPE.names == paircontactsmodel.SUMMARY_NAMES and gpu.PAIR_CONTACTS_MAX_PAIRS == 65536


# ---- the sanitizer build ------------------------------------------------------------------------------------------------------------------------

def test_the_rules_run_clean_under_the_sanitizers(rules, tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python) built with -fsanitize=address,undefined: the argument checks,
    the box pairs and the scenes with clipped boxes, tall boxes and empty intersections run to the end and give the bytes of the plain build."""
    program = ruleslib.build("pair_contacts_rules", tmp_path, *SANITIZE)
    _check_args(subprocess.check_output([program, "args"], text=True))
    boxes = tmp_path / "boxes"
    boxes.mkdir()
    _check_box_pairs(program, boxes)
    cases = [scene_cubes(), scene_steps(), scene_clipped(), scene_empty(), scene_empty(True), scene_lattice(3)]
    want = [model_of(*c) for c in cases]
    plain, clean = tmp_path / "plain", tmp_path / "clean"
    plain.mkdir()
    clean.mkdir()
    for g, w in zip(run_cases(program, clean, cases), want):
        same(g, w, "the sanitizer build")
    for g, w in zip(run_cases(rules, plain, cases), want):
        same(g, w, "the plain build")
