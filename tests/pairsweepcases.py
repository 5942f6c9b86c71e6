"""The cases of cvxm_pair_sweep that tests/test_model_sweep_cpu.py runs through the host rules and tests/test_gpu_model_sweep.py through the
device, and the answer of tests/pairsweepmodel.py for each, computed once.

  CASES        -> name: a function that gives (models, instances, pairs, motions)
  case(name), answer(name) -> the case and the model's (sweeps, contacts, summary), both cached
  property_of(name)        -> asserts, from the model's answer alone, the property the case is named for"""
from __future__ import annotations

import functools

import numpy as np

import pairsweepmodel
import sweepmodel
from cpuvox_amd import gpu
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, make_instance, random_model, rotation, tilt

FILL = gpu.BRUSH_FILL
PLATE, VOXEL, CUBE = (8, 1, 8), (1, 1, 1), (2, 2, 2)
TIES = {"2 2 2": ((2, 2, 2), 2), "3 -1 2": ((3, -1, 2), 4), "-5 7 -3": ((-5, 7, -3), 8)}  # the motion and the pose at which the other voxel waits
HEIGHTS = (1, 64, 65, 200, 300)
COUNTS = (1, 64, 65, 4097, 65536)


def _full(size, argb=0xFF445566):
    return (np.full((size[0], size[2], size[1]), argb, dtype=np.uint32), None)


def _only(size, voxels, mask=False):
    """A model of `size` whose set voxels are `voxels` (x, y, z); with `mask` every colour is set and the mask says which voxels are."""
    argb = np.zeros((size[0], size[2], size[1]), dtype=np.uint32)
    solid = np.zeros(argb.shape, dtype=np.uint8)
    for x, y, z in voxels:
        argb[x, z, y], solid[x, z, y] = 0xFF99AA11, 1
    return (np.full(argb.shape, 0xFF010203, dtype=np.uint32), solid) if mask else (argb, None)


def _plates(ya, yb, motion):
    return [_full(PLATE)], [identity_at((4, ya, 4), PLATE, 0, FILL), identity_at((4, yb, 4), PLATE, 0, FILL)], [(0, 1)], [motion]


def _axis(name):
    """Two cubes nine voxels apart along the axis: a moves twelve towards b; and b towards a by the opposite motion."""
    axis, sign = "xyz".index(name[1]), (1 if name[0] == "+" else -1)
    at, v = [20, 20, 20], [0, 0, 0]
    at[axis] -= 11 * sign
    v[axis] = 12 * sign
    return [_full(CUBE)], [identity_at(at, CUBE, 0, FILL), identity_at((20, 20, 20), CUBE, 0, FILL)], [(0, 1), (1, 0)], [v, [-c for c in v]]


def _tie(name):
    """One voxel that waits at pose j of the motion's path for one that starts at the origin of it: any other order of the tied steps passes it by."""
    v, j = TIES[name]
    there = sweepmodel.path(v)[j][0]
    start = (7, 9, 5)
    return ([_full(VOXEL)], [identity_at(start, VOXEL, 0, FILL), identity_at([start[c] + there[c] for c in range(3)], VOXEL, 0, FILL)], [(0, 1), (1, 0)],
            [list(v), [-c for c in v]])


MAPS = {"yaw 30": rotation(1, 30), "tilt": tilt(), "scale 1.5": 1.5 * rotation(1, 30), "scale 1/2": 0.5 * np.eye(3), "mirror": np.diag([-1.0, 1.0, 1.0]) @ rotation(1, 15)}


def _maps():
    """Every map on a, against a tilted b; then every map on b, against a yawed a.  One model has a mask, the other colours alone."""
    rng = np.random.default_rng(77)
    size_a, size_b = (5, 6, 4), (6, 4, 7)
    models = [random_model(rng, size_a, with_mask=True, zeros=0.3), random_model(rng, size_b, zeros=0.3)]
    instances, pairs, motions = [], [], []
    for k, linear in enumerate(MAPS.values()):
        cx = 40.0 * k
        v = [(7, -9, 3), (-6, 8, 5), (9, 4, -8), (-5, -7, -6), (8, 8, 8)][k]
        for moving, fixed, m_model, f_model in ((linear, tilt(), 0, 1), (rotation(1, 30), linear, 1, 0)):
            size_m, size_f = (size_a, size_b) if m_model == 0 else (size_b, size_a)
            centre = np.array([cx, 20.0 if m_model == 0 else 60.0, 10.0])
            instances.append(gpu.model_instance(forward_about_centre(fixed, size_f, centre + 0.3), size_f, f_model, FILL))
            instances.append(gpu.model_instance(forward_about_centre(moving, size_m, centre - 0.7 * np.asarray(v) + 0.1), size_m, m_model, FILL))
            pairs.append((len(instances) - 1, len(instances) - 2))
            motions.append(v)
    return models, instances, pairs, motions


def _boxes():
    """A box larger than its body, and set model voxels whose image lies outside their instance's own box.  Every pair moves (0, 8, 0); the row
    models are four voxels along x.  Pair 0: a full row in a box ten voxels wider on every side comes up under the one set voxel (x = 3) of b's
    row: hit 5.  Pair 1: the same with a's box cut to x in [0, 2): its voxel x = 3 does not count.  Pair 2: a's one voxel x = 3 under a full row
    whose box is cut to x in [0, 2).  Pair 3: pair 2 with the box whole: hit 5."""
    row = (4, 1, 1)
    models = [_full(row), _only(row, [(3, 0, 0)])]
    one = np.eye(3, dtype=np.int64) * 65536
    wide = make_instance(one, [0, 0, 0], (-10, -10, -10), (14, 11, 11), 0, FILL)
    cut = make_instance(one, [0, 0, 0], (0, 0, 0), (2, 1, 1), 0, FILL)
    cut_above = make_instance(one, [0, -5 * 65536, 0], (0, 5, 0), (2, 6, 1), 0, FILL)
    instances = [wide, identity_at((0, 5, 0), row, 1, FILL), cut, identity_at((0, 0, 0), row, 1, FILL), cut_above, identity_at((0, 5, 0), row, 0, FILL)]
    return models, instances, [(0, 1), (2, 1), (3, 4), (3, 5)], [(0, 8, 0)] * 4


def _column(height):
    """A full column of `height` voxels falls onto one voxel: the only touching voxel is its lowest, in the last of its steps of 64."""
    size = (1, height, 1)
    return [_full(size), _full(VOXEL)], [identity_at((3, 20, 3), size, 0, FILL), identity_at((3, 11, 3), VOXEL, 1, FILL)], [(0, 1)], [(0, -12, 0)]


def _lane(lane):
    """A 64-voxel box whose only body voxel is lane `lane` of its one step (lane 0 the top), falling onto a plate."""
    size = (1, 64, 1)
    return [_only(size, [(0, 63 - lane, 0)]), _full(PLATE)], [identity_at((6, 20, 6), size, 0, FILL), identity_at((4, 10, 4), PLATE, 1, FILL)], [(0, 1)], [(0, -80, 0)]


def _windows():
    """Pair 0: the one column of a can come over b's box on x (late: b lies three to its right) and on z (early: it leaves b's one row at once),
    never on both: a job whose window is empty.  Pair 1: a column straight above b, its window the whole path."""
    models = [_full(VOXEL)]
    instances = [identity_at((0, 5, 0), VOXEL, 0, FILL), identity_at((3, 5, 0), VOXEL, 0, FILL), identity_at((20, 9, 20), VOXEL, 0, FILL), identity_at((20, 3, 20), VOXEL, 0, FILL)]
    return models, instances, [(0, 1), (2, 3)], [(4, 0, 4), (0, -8, 0)]


def _later_step(both=True):
    """A column of 130 voxels moves six along +x; b's lowest voxel waits three away, its highest six away: the column's first step of 64 (the
    top) finds pose 6, its last finds pose 3.  both=False: b without its lowest voxel."""
    size_a, size_b = (1, 130, 1), (6, 130, 1)
    voxels = [(5, 129, 0)] + ([(2, 0, 0)] if both else [])
    return [_full(size_a), _only(size_b, voxels, mask=True)], [identity_at((0, 0, 0), size_a, 0, FILL), identity_at((1, 0, 0), size_b, 1, FILL)], [(0, 1)], [(6, 0, 0)]


def _voxels(count, seed):
    """`count` pairs among twelve one-voxel bodies in a small cube: every round of the search for the pair, and the limit.  Two motions in five
    end on the other voxel, two pass a voxel beside it, one goes the other way and has no job."""
    rng = np.random.default_rng(seed)
    spots = rng.permutation(5 * 5 * 5)[:12]
    at = np.array([(int(s) // 25, int(s) // 5 % 5, int(s) % 5) for s in spots])
    instances = [identity_at(tuple(int(c) for c in spot), VOXEL, 0, FILL) for spot in at]
    a = rng.integers(0, 12, size=count)
    b = (a + rng.integers(1, 12, size=count)) % 12
    towards, kind = at[b] - at[a], rng.integers(0, 5, size=count)
    beside = np.array([(0, 0, 0), (0, 0, 0), (1, 0, 0), (0, -1, 0)])
    motions = np.where((kind == 4)[:, None], -towards, towards + beside[np.minimum(kind, 3)])
    return [_full(VOXEL)], instances, np.stack([a, b], axis=-1).astype(np.int32), motions


def _repeats():
    """The same pair twice with different motions; then one instance in 50 pairs; a pair with no jobs between two with jobs."""
    rng = np.random.default_rng(5)
    models = [_full(CUBE), random_model(rng, (4, 5, 3), zeros=0.2)]
    instances = [identity_at((0, 0, 0), (4, 5, 3), 1, FILL)]
    for k in range(50):
        instances.append(identity_at((int(rng.integers(-9, 10)), int(rng.integers(-9, 10)), int(rng.integers(-9, 10))), CUBE, 0, FILL))
    pairs = [(1, 0), (1, 0)] + [(k, 0) if k % 2 else (0, k) for k in range(1, 51)]
    motions = [(-int(instances[1].boxMin[0]), -int(instances[1].boxMin[1]), -int(instances[1].boxMin[2])), (3, 3, 3)]
    for a, b in pairs[2:]:
        towards = [int(instances[b].boxMin[c]) - int(instances[a].boxMin[c]) for c in range(3)]
        motions.append(towards if (a + b) % 3 else [-c for c in towards])  # every third moves away: no jobs
    return models, instances, pairs, motions


def _long(miss):
    """One voxel goes (4096, -5, 2); the other waits at pose 4090 of that path -- or, for the miss, a voxel beside it."""
    v = (4096, -5, 2)
    there = list(sweepmodel.path(v)[4090][0])
    there[1] += 1 if miss else 0
    return [_full(VOXEL)], [identity_at((0, 0, 0), VOXEL, 0, FILL), identity_at(there, VOXEL, 0, FILL)], [(0, 1)], [v]


FUZZ_SEED, FUZZ_PAIRS, FUZZ_BODIES = 20264, 300, 48


def _fuzz():
    """300 pairs of random bodies of 3 .. 9 voxels a side under random maps, motions within [-12, 12]^3."""
    rng = np.random.default_rng(FUZZ_SEED)
    sizes = [tuple(int(c) for c in rng.integers(3, 10, size=3)) for _ in range(6)]
    models = [random_model(rng, size, with_mask=bool(k % 2), zeros=0.35) for k, size in enumerate(sizes)]
    linears = [np.eye(3), rotation(1, 30), tilt(), 1.5 * rotation(1, 45), 0.5 * np.eye(3), np.diag([1.0, -1.0, 1.0]) @ rotation(2, 20), rotation(0, 90)]
    instances, centres = [], []
    for _ in range(FUZZ_BODIES):
        k = int(rng.integers(0, len(models)))
        linear = linears[int(rng.integers(0, len(linears)))]
        centres.append(rng.uniform(0, 22, size=3))
        instances.append(gpu.model_instance(forward_about_centre(linear, sizes[k], centres[-1]), sizes[k], k, FILL))
    a = rng.integers(0, FUZZ_BODIES, size=FUZZ_PAIRS)
    b = (a + rng.integers(1, FUZZ_BODIES, size=FUZZ_PAIRS)) % FUZZ_BODIES
    # three motions in four head for the other body, give or take three voxels, and stop short of it or go beyond; the others go anywhere
    centres = np.asarray(centres)
    aimed = np.rint((centres[b] - centres[a]) * rng.uniform(0.3, 1.3, size=(FUZZ_PAIRS, 1))).astype(np.int64) + rng.integers(-3, 4, size=(FUZZ_PAIRS, 3))
    anywhere = rng.integers(-12, 13, size=(FUZZ_PAIRS, 3))
    motions = np.clip(np.where((rng.integers(0, 4, size=FUZZ_PAIRS) > 0)[:, None], aimed, anywhere), -12, 12)
    return models, instances, np.stack([a, b], axis=-1).astype(np.int32), motions


CASES = {
    # the thin shell and the ends of the range
    "thin shell": lambda: _plates(9, 5, (0, -8, 0)),
    "starts overlapping": lambda: _plates(5, 5, (0, -3, 0)),
    "hit at n": lambda: _plates(9, 5, (0, -4, 0)),
    "miss by one": lambda: _plates(9, 5, (0, -3, 0)),
    "still": lambda: ([_full(PLATE)], [identity_at((4, 9, 4), PLATE, 0, 0), identity_at((4, 5, 4), PLATE, 0, 0), identity_at((6, 5, 0), PLATE, 0, 0)], [(0, 1), (2, 1)],
                      [(0, 0, 0), (0, 0, 0)]),
    # the path
    **{name: functools.partial(_axis, name) for name in ("-x", "+x", "-y", "+y", "-z", "+z")},
    **{name: functools.partial(_tie, name) for name in TIES},
    # maps and boxes
    "maps": _maps,
    "boxes": _boxes,
    # waves
    **{f"column {h}": functools.partial(_column, h) for h in HEIGHTS},
    "lane 0": lambda: _lane(0),
    "lane 63": lambda: _lane(63),
    "windows": _windows,
    "later step": _later_step,
    # pairs
    **{f"{n} pairs": functools.partial(_voxels, n, n) for n in COUNTS},
    "repeats": _repeats,
    # the long motion
    "long hit": lambda: _long(False),
    "long miss": lambda: _long(True),
    # fuzz
    "fuzz": _fuzz,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def answer(name):
    models, instances, pairs, motions = case(name)
    return pairsweepmodel.sweep(models, as_dicts(instances), pairs, motions)


def _ends(name, p=0):
    """The model's overlap of pair p at its two end poses."""
    models, instances, pairs, motions = case(name)
    a, b = (int(k) for k in pairs[p])
    dicts = as_dicts(instances)
    return [int(pairsweepmodel.paircontactsmodel.contacts(models, [sweepmodel.moved(dicts[a], o), dicts[b]], [(0, 1)])[0]["overlap"][0]) for o in ((0, 0, 0), motions[p])]


def property_of(name):
    """What the case is named for, asserted from the model's answer alone (the GPU test asserts it too, before it asks the device)."""
    models, instances, pairs, motions = case(name)
    sweeps, contacts, summary = answer(name)
    s = sweeps["sweep"]
    first = s[0]
    if name == "thin shell":
        assert _ends(name) == [0, 0], "no overlap at either end pose: the plate passes through the plate"
        assert (first["hit"], first["axis"], first["sign"], first["steps"]) == (4, 1, -1, 8) and first["free"].tolist() == [0, -3, 0] and first["at"].tolist() == [0, -4, 0]
        assert contacts["overlap"][0] == 64 and contacts["pushA"][0].tolist() == [0, 0, 0], "a voxel thick: both faces of every overlap voxel are open"
    elif name == "starts overlapping":
        assert (first["hit"], first["axis"], first["sign"]) == (0, -1, 0) and not first["free"].any() and not first["at"].any() and summary["startsSolid"] == 1
    elif name == "hit at n":
        assert first["hit"] == first["steps"] == 4 and first["at"].tolist() == [0, -4, 0]
    elif name == "miss by one":
        assert (first["hit"], first["axis"], first["sign"]) == (-1, -1, 0) and first["free"].tolist() == first["at"].tolist() == [0, -3, 0] and contacts["overlap"][0] == 0
    elif name == "still":
        assert s["steps"].tolist() == [0, 0] and s["hit"].tolist() == [-1, 0] and not s["at"].any() and summary["jobs"] == 6 * 4
    elif name in ("-x", "+x", "-y", "+y", "-z", "+z"):
        axis, sign = "xyz".index(name[1]), (1 if name[0] == "+" else -1)
        assert s["hit"].tolist() == [10, 10] and s["axis"].tolist() == [axis, axis] and s["sign"].tolist() == [sign, -sign] and _ends(name)[0] == 0
    elif name in TIES:
        v, j = TIES[name]
        axes = [a for _, a in sweepmodel.path(v)]
        assert s["hit"].tolist() == [j, j] and s["axis"].tolist() == [axes[j]] * 2 and _ends(name) == [0, 0], "the other voxel lies on the path, not at its end"
        tied = {"2 2 2": [0, 1, 2], "3 -1 2": [0, 1], "-5 7 -3": [0, 1, 2]}[name]
        at = j - tied.index(axes[j])
        assert axes[at:at + len(tied)] == tied, "equal parameters: the lower axis first"
        assert len(tied) > 1 and axes[j] != 0, "x first would not tell: the voxel waits behind a step that lost a tie"
    elif name == "maps":
        assert (s["hit"] > 0).sum() >= 6 and len(pairs) == 10, "most of the ten meet on the way"
        volumes = [int(pairsweepmodel.contactsmodel.body(models, d).sum()) for d in as_dicts(instances)]
        assert min(volumes) > 0 and len(set(volumes)) >= 6, "scales 1.5 and 1/2 give other bodies"
        assert models[0][1] is not None and models[1][1] is None
    elif name == "boxes":
        assert s["hit"].tolist() == [5, -1, -1, 5] and summary["jobs"] > 4, "the cut boxes have jobs: they are walked and find nothing"
    elif name.startswith("column "):
        height = int(name.split()[1])
        assert instances[0].boxMax[1] - instances[0].boxMin[1] == height and first["hit"] == 9 and contacts["overlap"][0] == 1
        assert contacts["min"][0].tolist() == [3, 11, 3] and (height > 4 * 64) == (name == "column 300"), "the lowest voxel; the last is past the plain-steps cut"
    elif name in ("lane 0", "lane 63"):
        assert first["hit"] == (73 if name == "lane 0" else 10) and contacts["overlap"][0] == 1
    elif name == "windows":
        assert s["hit"].tolist() == [-1, 6] and summary["jobs"] == 2, "both pairs have their one job"
    elif name == "later step":
        alone = pairsweepmodel.sweep(*_later_step(both=False)[:1], as_dicts(_later_step(both=False)[1]), [(0, 1)], [(6, 0, 0)], want_contacts=False)[0]
        assert first["hit"] == 3 and alone["sweep"]["hit"][0] == 6 and contacts["min"][0].tolist() == [3, 0, 0]
    elif name.endswith(" pairs"):
        assert len(pairs) == int(name.split()[0]) and (np.asarray(pairs)[:, 0] != np.asarray(pairs)[:, 1]).all()
        if len(pairs) >= 64:
            assert (s["hit"] > 0).any() and (s["hit"] == -1).any() and summary["jobs"] < len(pairs), "some pairs have no job"
    elif name == "repeats":
        assert tuple(pairs[0]) == tuple(pairs[1]) and s["hit"][0] >= 0 and tuple(s["at"][0]) != tuple(s["at"][1])
        assert sum(1 for a, b in pairs if 0 in (a, b)) == 52
        per_pair = [pairsweepmodel.pair_jobs(as_dicts(instances)[a], as_dicts(instances)[b], v) for (a, b), v in zip(pairs, motions)]
        assert any(per_pair[k - 1] and not per_pair[k] and per_pair[k + 1] for k in range(1, len(pairs) - 1)), "a pair with no jobs between two with jobs"
        assert (contacts["firstPoint"][1:] >= contacts["firstPoint"][:-1]).all() and contacts["firstPoint"][-1] > 0
    elif name == "long hit":
        assert first["hit"] == 4090 and first["steps"] == 4103
    elif name == "long miss":
        assert first["hit"] == -1 and first["at"].tolist() == [4096, -5, 2] and summary["jobs"] == 1
    elif name == "fuzz":
        hits = s["hit"]
        assert len(hits) == FUZZ_PAIRS
        assert (hits > 0).mean() >= 0.20 and (hits == -1).mean() >= 0.10 and (hits == 0).mean() >= 0.05, ((hits > 0).mean(), (hits == -1).mean(), (hits == 0).mean())
    else:
        raise AssertionError(f"no property for {name}")
