"""Test infrastructure (numpy and scipy only, no device): the calls of tests/test_gpu_model_kernel_limits.py and tests/test_gpu_model_sequences.py, the
placed-model calls (cvxp_model_contacts, cvxq_model_pick, cvxc_world_contacts) at their kernels' compiled limits, TOGETHER with the counts and
properties each case is named after, computed from the numpy models, the host rules programs or plain arithmetic
(tests/test_limit_models_cpu.py checks them on the CPU; the GPU tests repeat the cheap ones before they call the device).

The limits are constants of the .hip files: the 1024 threads of the finish kernel (64 pairs each), the 64 probes a round of the pair search
(three rounds above 4096 pairs, a first probe step of 1024 at 65536), the 4096 counts of a scan chunk (one count per 64 (ray, instance) pairs),
the 4096 instances of a call, the 64 layers of a pick step, and +-2^30, the last coordinate the validation lets through."""
from __future__ import annotations

import functools

import numpy as np

import paircontactsmodel
from cpuvox_amd import gpu
from test_model_contacts_cpu import FILL, model_of, scene_cubes
from test_model_pick_cpu import rays_of
from test_world_contacts_cpu import CUBE, cube_model
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, make_instance, random_model, rotation, tilt

LIMIT = 1 << 30
WAVE = 64
FINISH_THREADS, PAIRS_EACH = 1024, 64  # cvxi::FinishResults<CVXP_MAX_PAIRS, 2>: thread t finishes pairs 64 t .. 64 t + 63
PROBE_STEP = 1024                      # the first round's probe step at 65536 pairs
SCAN_CHUNK = 4096                      # CVX_SCAN_CHUNK


def moved(instances, delta):
    """Copies of `instances` moved by the integer vector `delta`: the boxes shifted, toModel's t taken back through m."""
    out = []
    for inst in instances:
        m = [[int(inst.toModel.m[i][j]) for j in range(3)] for i in range(3)]
        t = [int(inst.toModel.t[i]) - sum(m[i][j] * int(delta[j]) for j in range(3)) for i in range(3)]
        out.append(make_instance(m, t, [int(inst.boxMin[i]) + int(delta[i]) for i in range(3)], [int(inst.boxMax[i]) + int(delta[i]) for i in range(3)], inst.model, inst.op))
    return out


# ---- A1. pair counts at the finish kernel's and the pair search's limits ------------------------------------------------------------------------------

PAIR_COUNTS = (64, 65, 4096, 4097, 65536)
RUN_LENGTH = 1100  # of consecutive empty pairs: longer than PROBE_STEP


@functools.lru_cache(maxsize=None)
def lattice_base():
    """(models, instances, base pairs, D, the model's answer for the base pairs): 27 cubes of 3 x 3 x 3 spaced two apart, every one with a model of its
    own, and two instances far away.  The first D base pairs are the lattice's box_pairs (neighbours share a layer, a line or a voxel; some of
    those do not meet); the last two pair a cube with a far instance: their boxes do not intersect, so they have no job."""
    rng = np.random.default_rng(8)
    models = [random_model(rng, (3, 3, 3), zeros=0.1) for _ in range(27)]
    instances = [identity_at((2 * x, 2 * y, 2 * z), (3, 3, 3), 9 * x + 3 * y + z, FILL) for x in range(3) for y in range(3) for z in range(3)]
    pairs = paircontactsmodel.box_pairs(as_dicts(instances))
    instances += [identity_at((500, 7, -90), (3, 3, 3), 0, FILL), identity_at((-40, -300, 12), (3, 3, 3), 5, FILL)]
    base = np.concatenate([pairs, np.int32([[3, 27], [28, 13]])])
    return models, instances, base, len(pairs), model_of(models, instances, base)


def empty_runs(count):
    """The runs [from, to) of consecutive empty pairs of the call of `count` pairs: three of them at 65536, the first at the start of the list,
    the second across a multiple of 1024 in the middle, the third at the end; one short run inside the smaller calls."""
    if count == 65536:
        return [(0, RUN_LENGTH), (32 * PROBE_STEP - 500, 32 * PROBE_STEP + 700), (count - RUN_LENGTH, count)]
    return [(count // 3, count // 3 + 3)]


def cycled_which(count, runs):
    """For every pair of a call its index into lattice_base()'s base pairs: the D distinct pairs in turn, inside a run the two empty ones."""
    d = lattice_base()[3]
    which = np.arange(count) % d
    for lo, hi in runs:
        which[lo:hi] = d + np.arange(hi - lo) % 2
    return which


def cycled_call(count, runs=None):
    """(models, instances, pairs, which) of the call of `count` pairs that cycles through the lattice's D distinct pairs."""
    models, instances, base, _, _ = lattice_base()
    which = cycled_which(count, empty_runs(count) if runs is None else runs)
    return models, instances, np.ascontiguousarray(base[which]), which


def pair_jobs(instances, pairs):
    """Per pair the (pair, column) jobs: the footprint of the two boxes' intersection, 0 where it is empty (plain arithmetic)."""
    lo = np.array([list(i.boxMin) for i in instances], dtype=np.int64)
    hi = np.array([list(i.boxMax) for i in instances], dtype=np.int64)
    pairs = np.asarray(pairs).reshape(-1, 2)
    size = np.minimum(hi[pairs[:, 0]], hi[pairs[:, 1]]) - np.maximum(lo[pairs[:, 0]], lo[pairs[:, 1]])
    return np.where((size > 0).all(axis=1), size[:, 0] * size[:, 2], 0)


def tile_answer(base_answer, base_jobs, which):
    """The model's answer of the call whose pair p is base pair which[p], from the model's answer for the base pairs: the results gathered,
    firstPoint the running sum of the points before, every pair's points copied with their `pair` rewritten, the summary added up."""
    base_results, base_points, _ = base_answer
    which = np.asarray(which)
    results = base_results[which].copy()
    counts = results["points"].astype(np.int64)
    first = np.cumsum(counts) - counts
    results["firstPoint"] = first
    total = int(counts.sum())
    source = np.repeat(base_results["firstPoint"][which].astype(np.int64) - first, counts) + np.arange(total)
    points = base_points[source].copy()
    points["pair"] = np.repeat(np.arange(len(which), dtype=np.int32), counts)
    summary = dict(touching=int((results["overlap"] > 0).sum()), overlap=int(results["overlap"].sum()), points=total, jobs=int(np.asarray(base_jobs)[which].sum()))
    return results, points, summary


@functools.lru_cache(maxsize=None)
def cycled_answer(count):
    """The call of `count` pairs and its answer: (models, instances, pairs, which, (results, points, summary))."""
    models, instances, pairs, which = cycled_call(count)
    _, _, base, _, base_answer = lattice_base()
    return models, instances, pairs, which, tile_answer(base_answer, pair_jobs(instances, base), which)


def job_prefix(instances, pairs):
    """The prefix the pair search runs over: the jobs before every pair, and all of them last."""
    return np.concatenate([[0], np.cumsum(pair_jobs(instances, pairs))])


def assert_cycled(count, call):
    """What the call of `count` pairs is named after, from the model's answer and plain arithmetic."""
    models, instances, pairs, which, (results, points, summary) = call
    d = lattice_base()[3]
    assert len(pairs) == count == len(results) and summary["points"] == len(points) < 1000000
    runs = empty_runs(count)
    prefix = job_prefix(instances, pairs)
    assert prefix[-1] == summary["jobs"] and (np.diff(prefix) >= 0).all()
    in_run = np.zeros(count, dtype=bool)
    for lo, hi in runs:
        in_run[lo:hi] = True
        assert (prefix[lo:hi + 1] == prefix[lo]).all() and not results["overlap"][lo:hi].any(), "a run of empty pairs: the prefix holds one value"
    assert (np.diff(prefix)[~in_run] > 0).all() and (results["overlap"][~in_run] > 0).sum() > 0.7 * (~in_run).sum()
    threads = -(-count // PAIRS_EACH)
    assert threads == min(FINISH_THREADS, threads) and (count < 4096 or threads > 32), "the finish kernel's threads that hold pairs"
    assert (count > 4096) == (count in (4097, 65536)), "above 4096 pairs the search takes three rounds"
    if count == 65536:
        assert threads == FINISH_THREADS and len(runs) == 3 and all(hi - lo >= RUN_LENGTH > PROBE_STEP for lo, hi in runs)
        assert runs[0][0] == 0 and runs[2][1] == count and runs[1][0] // PROBE_STEP < (runs[1][1] - 1) // PROBE_STEP and 0 < runs[1][0] and runs[1][1] < count
        blocks = np.arange(count).reshape(FINISH_THREADS, PAIRS_EACH)
        outside = ~in_run[blocks].any(axis=1)
        assert outside.sum() > 900 and (results["points"][blocks[outside]] > 0).any(axis=1).all(), "every block of 64 pairs outside the runs holds a pair with points"
        first = results["firstPoint"][blocks[:, 0]]
        grows = first[1:] > first[:-1]
        assert grows[outside[:-1]].all(), "firstPoint grows across every block boundary outside the runs"
        assert (np.diff(results["firstPoint"]) >= 0).all() and results["firstPoint"][-1] + results["points"][-1] == summary["points"]
    assert set(which[~in_run].tolist()) == set(range(min(d, count))) or count < d


def assert_lattice_base():
    models, instances, base, d, (results, points, summary) = lattice_base()
    assert d == 158 and len(base) == d + 2
    met = results["overlap"][:d]
    assert set(met.tolist()) >= {0} and (met >= 6).any() and ((met > 0) & (met <= 3)).any() and (met == 1).any(), "a layer, a line, a voxel, and pairs that do not meet"
    assert not results["overlap"][d:].any() and (pair_jobs(instances, base)[d:] == 0).all() and (pair_jobs(instances, base)[:d] > 0).all()
    touching = results[:d][met > 0]
    fields = ("overlap", "points", "sum", "pushA", "pushB", "origin", "min", "max")  # (all but the pair's own indices and its place in the list)
    keys = {tuple(np.concatenate([np.atleast_1d(r[f]).astype(np.int64) for f in fields]).tolist()) for r in touching}
    assert len(keys) == len(touching), "no two distinct pairs have equal results"
    assert len({instances[k].model for k in range(27)}) == 27


# ---- A3. boxes at +-2^30 ---------------------------------------------------------------------------------------------------------------------------

def _tall_pair(low):
    """A cube and a tilted small body that meet, in boxes 500 tall whose bottom is y = 0 (low) or whose top is y = 500, the bodies next to that end:
    (models, instances, pairs) at the origin."""
    rng = np.random.default_rng(31)
    models = [cube_model(), random_model(rng, (5, 6, 4), zeros=0.2)]
    y = 6 if low else 492
    instances = [identity_at((20, y, 20), CUBE, 0, FILL), gpu.model_instance(forward_about_centre(tilt(), (5, 6, 4), (22, y + 2, 22)), (5, 6, 4), 1, FILL)]
    for inst in instances:
        inst.boxMin[1], inst.boxMax[1] = 0, 500
    return models, instances, np.int32([[0, 1], [1, 0]])


def limit_pair_cases():
    """[(name, the scene at the origin, the scene moved to the limit, the move)]: scene_cubes() with its boxes ending exactly at +2^30 on each axis,
    beginning exactly at -2^30 on each axis and in the corner (-2^30, -2^30, -2^30); two pairs with boxes 500 tall that begin at y = -2^30 and end
    at y = 2^30."""
    cases = []
    models, instances, pairs = scene_cubes()
    lo = [min(int(i.boxMin[a]) for i in instances) for a in range(3)]
    hi = [max(int(i.boxMax[a]) for i in instances) for a in range(3)]
    for axis in range(3):
        delta = [0, 0, 0]
        delta[axis] = LIMIT - hi[axis]
        cases.append((f"ends at +2^30 on axis {axis}", (models, instances, pairs), delta))
    for axis in range(3):
        delta = [0, 0, 0]
        delta[axis] = -LIMIT - lo[axis]
        cases.append((f"begins at -2^30 on axis {axis}", (models, instances, pairs), delta))
    cases.append(("the corner at -2^30", (models, instances, pairs), [-LIMIT - lo[a] for a in range(3)]))
    cases.append(("500 tall from y = -2^30", _tall_pair(True), [3, -LIMIT, -7]))
    cases.append(("500 tall up to y = 2^30", _tall_pair(False), [-5, LIMIT - 500, 11]))
    return [(name, scene, (scene[0], moved(scene[1], delta), scene[2]), delta) for name, scene, delta in cases]


def shifted_answer(answer, delta):
    """A pair answer at the origin -> the answer after a move by `delta`: voxel, origin, min and max shifted (min and max only where there is an
    overlap: without one they are zeros), everything else unchanged."""
    results, points, summary = answer
    results, points = results.copy(), points.copy()
    d = np.int32(delta)
    results["origin"] += d
    met = results["overlap"] > 0
    results["min"][met] += d
    results["max"][met] += d
    points["voxel"] += d
    return results, points, dict(summary)


def assert_limit_pair(name, at_limit, delta):
    models, instances, pairs = at_limit
    lo = np.array([list(i.boxMin) for i in instances], dtype=np.int64)
    hi = np.array([list(i.boxMax) for i in instances], dtype=np.int64)
    assert (lo >= -LIMIT).all() and (hi <= LIMIT).all() and ((lo == -LIMIT).any() or (hi == LIMIT).any()), name
    if "tall" in name:
        assert (hi[:, 1] - lo[:, 1] == 500).all() and (lo[:, 1] == -LIMIT).all() != (hi[:, 1] == LIMIT).all(), name
    elif "corner" in name:
        assert lo.min(axis=0).tolist() == [-LIMIT] * 3
    else:
        axis = int(name[-1])
        assert (hi[:, axis].max() == LIMIT) if "ends" in name else (lo[:, axis].min() == -LIMIT), name
        if "ends" in name:
            assert max(hi[a, axis] for a in pairs[0]) == LIMIT, "the pair's boxes"


# ---- B1. pick: bodies deeper than 64 layers -------------------------------------------------------------------------------------------------------

LONG_LENGTHS = (65, 128, 129, 200, 320)
LONG_CROSS = (9, 7)
LONG_MAPS = {"identity": np.eye(3), "yaw 30": rotation(1, 30), "tilt": tilt(), "scale 2": 2.0 * np.eye(3), "scale 1/2": 0.5 * np.eye(3), "mirror": np.diag([1.0, 1.0, -1.0])}
DEEP_LAYERS = ((64, 50), (128, 50), (192, 20))  # (beyond this layer of the winning box, at least so many rays hit)


def boxed_instance(rng, linear, lo, hi, model_index, air):
    """(model, instance): a random body with `air` of its voxels empty under the map `linear` about the centre of the box [lo, hi), the model as
    large as the box's image in model space, so that the body fills the box from end to end.  Small models have colours, large ones a mask alone."""
    linear = np.asarray(linear, dtype=np.float64)
    half = np.abs(np.linalg.inv(linear)) @ ((np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)) / 2)
    size = tuple(int(v) for v in np.ceil(2 * half) + 2)
    shape = (size[0], size[2], size[1])
    mask = rng.random(shape) >= air
    if mask.size <= 300000:
        model = (np.where(mask, rng.integers(1, 1 << 32, shape, dtype=np.uint64), 0).astype(np.uint32), None)
    else:
        model = (None, mask)
    inst = gpu.model_instance(forward_about_centre(linear, size, (np.asarray(lo) + np.asarray(hi)) / 2.0), size, model_index, FILL)
    for a in range(3):
        inst.boxMin[a], inst.boxMax[a] = int(lo[a]), int(hi[a])
    return model, inst


def _through_boxes(rng, boxes, axis, n):
    """n rays aimed through random points of the boxes, dominant along `axis` in both directions, the two minor-to-major slopes from 0.001 to 1."""
    b, c = [a for a in range(3) if a != axis]
    which = rng.integers(0, len(boxes), size=n)
    lo, hi = boxes[which, 0].astype(np.float64), boxes[which, 1].astype(np.float64)
    through = lo + rng.uniform(0.0, 1.0, size=(n, 3)) * (hi - lo)
    d = np.zeros((n, 3))
    d[:, axis] = rng.choice([-1.0, 1.0], size=n)
    for minor in (b, c):
        d[:, minor] = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-3.0, 0.0, size=n)
    back = np.where(d[:, axis] > 0, through[:, axis] - lo[:, axis], hi[:, axis] - through[:, axis]) + rng.uniform(1.0, 6.0, size=n)
    return through - d * back[:, None], d


@functools.lru_cache(maxsize=None)
def long_bodies(axis):
    """(models, instances, rays, the rays that are random): boxes 65 .. 320 layers long along `axis` with a cross-section of 9 x 7, one per length
    and map, side by side; 2048 random rays through them, 256 whose two largest components are exactly equal, 256 made of ties (origins on the
    half-voxel grid, components from powers of two)."""
    rng = np.random.default_rng(500 + axis)
    b, c = [a for a in range(3) if a != axis]
    models, instances = [], []
    for i, length in enumerate(LONG_LENGTHS):
        for j, linear in enumerate(LONG_MAPS.values()):
            lo = [0, 0, 0]
            lo[axis], lo[b], lo[c] = -37 + 11 * j - 5 * i, -20 + (LONG_CROSS[0] + 2) * j, -9 + (LONG_CROSS[1] + 1) * i
            hi = list(lo)
            hi[axis], hi[b], hi[c] = lo[axis] + length, lo[b] + LONG_CROSS[0], lo[c] + LONG_CROSS[1]
            model, inst = boxed_instance(rng, linear, lo, hi, len(models), 0.97 if length < 200 else 0.99)
            models.append(model)
            instances.append(inst)
    boxes = np.array([[list(i.boxMin), list(i.boxMax)] for i in instances])
    o1, d1 = _through_boxes(rng, boxes, axis, 2048)
    o2, d2 = _through_boxes(rng, boxes, axis, 256)
    d2[:, b] = np.where(np.arange(256) % 2 == 0, rng.choice([-1.0, 1.0], size=256) * np.abs(d2[:, axis]), d2[:, b])  # |d| equal on the two largest: the axis and b,
    d2[:, c] = np.where(np.arange(256) % 2 == 1, rng.choice([-1.0, 1.0], size=256) * np.abs(d2[:, axis]), d2[:, c])  # or the axis and c
    lo_all, hi_all = boxes[:, 0].min(axis=0), boxes[:, 1].max(axis=0)
    o3 = np.stack([rng.integers(2 * lo_all[a] - 8, 2 * hi_all[a] + 8, size=256) for a in range(3)], axis=-1) * 0.5
    d3 = rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=(256, 3))
    d3[:, axis] = np.where(np.arange(256) % 4 != 0, rng.choice([-2.0, 2.0], size=256), d3[:, axis])  # most of them along the bodies
    rays = rays_of(np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3]), 1e4)
    return models, instances, rays, np.arange(len(rays)) < 2048


def hit_layers(instances, rays, hits):
    """Per ray that hit: the layer of its winning box the hit lies in, counted from where the ray enters that box along the ray's dominant axis
    (the first of the largest |d|); -1 for a miss.  Plain float64 arithmetic of the slab test."""
    out = np.full(len(rays), -1, dtype=np.int64)
    for i in np.nonzero(hits["instance"] >= 0)[0]:
        inst = instances[int(hits["instance"][i])]
        o, d = rays["origin"][i].astype(np.float64), rays["direction"][i].astype(np.float64)
        major = int(np.argmax(np.abs(d)))
        t_enter = 0.0
        for a in range(3):
            if d[a] != 0.0:
                t_enter = max(t_enter, min((inst.boxMin[a] - o[a]) / d[a], (inst.boxMax[a] - o[a]) / d[a]))
        entered = min(max(int(np.floor(o[major] + t_enter * d[major])), int(inst.boxMin[major])), int(inst.boxMax[major]) - 1)
        out[i] = abs(int(hits["voxel"][i][major]) - entered)
    return out


def assert_long_bodies(cases, all_hits):
    """From the rules program's hits of the three calls: rays hit deep in their winning boxes."""
    layers = np.concatenate([hit_layers(case[1], case[2], hits) for case, hits in zip(cases, all_hits)])
    for beyond, at_least in DEEP_LAYERS:
        assert (layers > beyond).sum() >= at_least, f"{(layers > beyond).sum()} rays hit beyond layer {beyond} of their winning box"
    for case, hits in zip(cases, all_hits):
        sizes = np.array([list(i.boxMax) for i in case[1]]) - np.array([list(i.boxMin) for i in case[1]])
        assert sorted(set(sizes.max(axis=1).tolist())) == list(LONG_LENGTHS) and len(case[1]) == len(LONG_LENGTHS) * len(LONG_MAPS)
        assert set(hits["instance"].tolist()) >= set(range(len(case[1]))), "every box wins some ray"
        d = np.abs(case[2]["direction"])
        top = np.sort(d, axis=1)
        assert (top[2048:2304, 2] == top[2048:2304, 1]).all() and (top[:2048, 1] <= top[:2048, 2]).all() and (top[:2048, 1] / top[:2048, 2] > 0.5).sum() > 100


LONG_SUBSET = 512  # of the random rays: compared with tests/modelpickmodel.py


def long_subset(axis):
    """The 512 random rays of long_bodies(axis) the numpy model walks (every fourth)."""
    return np.arange(0, 2048, 4)


# ---- B2. pick: many jobs on one ray ---------------------------------------------------------------------------------------------------------------

ROW_SIZE = (200, 5, 5)


@functools.lru_cache(maxsize=None)
def crowded_row(reverse=False):
    """(models, instances, rays): 64 instances of one sparse 200 x 5 x 5 model (90 % air; its two end layers 30 % full) along x, four groups of 16 -- exact duplicates, copies shifted by
    1 .. 16 voxels along the row, copies shifted by a voxel or two across it, copies turned by 180 degrees about x, y or z -- and 512 rays along
    the row from both ends and on diagonals with power-of-two components.  reverse: the same call with the instance list reversed."""
    rng = np.random.default_rng(64)
    model = random_model(rng, ROW_SIZE, zeros=0.9)
    for end in (0, ROW_SIZE[0] - 1):  # the two end layers fuller: many rays end in the first layer of a box, at the very time they enter it
        model[0][end] = np.where(rng.random((ROW_SIZE[2], ROW_SIZE[1])) < 0.3, rng.integers(1, 1 << 32, (ROW_SIZE[2], ROW_SIZE[1]), dtype=np.uint64), 0).astype(np.uint32)
    at = (-30, 4, -6)
    centre = [at[a] + ROW_SIZE[a] / 2 for a in range(3)]
    across = [(dy, dz) for dy in (-2, -1, 1, 2) for dz in (-2, -1, 0, 1)]
    instances = []
    for k in range(16):
        instances.append(identity_at(at, ROW_SIZE, 0, FILL))
    for k in range(16):
        instances.append(identity_at((at[0] + k + 1, at[1], at[2]), ROW_SIZE, 0, FILL))
    for k in range(16):
        instances.append(identity_at((at[0], at[1] + across[k][0], at[2] + across[k][1]), ROW_SIZE, 0, FILL))
    for k in range(16):
        turned = [centre[0] + k // 3, centre[1], centre[2]]
        instances.append(gpu.model_instance(forward_about_centre(rotation(k % 3, 180), ROW_SIZE, turned), ROW_SIZE, 0, FILL))
    n = 512
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    cell = np.stack([rng.integers(0, 14, size=n), rng.integers(0, 14, size=n)], axis=-1) * 0.5 + 0.25  # off the planes, on a quarter-voxel grid
    up = np.arange(n) % 2 == 0
    o[:, 0] = np.where(up, at[0] - 8.0, at[0] + ROW_SIZE[0] + 24.0)
    o[:, 1], o[:, 2] = at[1] - 1 + cell[:, 0], at[2] - 1 + cell[:, 1]
    d[:, 0] = np.where(up, 1.0, -1.0)
    diagonal = np.arange(n) % 4 >= 2
    slope = rng.choice([-1 / 32, -1 / 64, -1 / 128, 1 / 128, 1 / 64, 1 / 32], size=(n, 2))
    d[diagonal, 1:] = slope[diagonal]
    rays = rays_of(o, d, 1e4)
    return [model], (instances[::-1] if reverse else instances), rays


def row_ties(run, case, hits):
    """The rays whose winner has an exact tie: `run` (cases -> [(hits, jobs)], the rules program) on the call without each ray's winner gives
    the same t, bit for bit."""
    models, instances, rays = case
    winners = sorted(set(hits["instance"][hits["instance"] >= 0].tolist()))
    cases, rows = [], []
    for k in winners:
        mine = np.nonzero(hits["instance"] == k)[0]
        cases.append((models, instances[:k] + instances[k + 1:], rays[mine]))
        rows.append(mine)
    tied = np.zeros(len(rays), dtype=bool)
    for mine, (second, _) in zip(rows, run(cases)):
        tied[mine] = (second["instance"] >= 0) & (second["t"].view(np.uint32) == hits["t"][mine].view(np.uint32))
    return tied


def assert_crowded_row(case, hits, jobs, tied):
    models, instances, rays = case
    assert len(instances) == 64 and len(rays) == 512 and len(models) == 1
    assert jobs >= 32 * len(rays), f"{jobs / len(rays):.1f} jobs a ray"
    winners = set(hits["instance"][hits["instance"] >= 0].tolist())
    assert len(winners) >= 24, f"the winners fall in {len(winners)} instances"
    assert tied.sum() >= 50, f"{tied.sum()} rays have an exact tie between instances"


# ---- B3. pick: the most instances and two scan chunks ---------------------------------------------------------------------------------------------

GRID_RAYS = 65


@functools.lru_cache(maxsize=None)
def cube_grid(copies=False):
    """(models, instances, rays): 4096 one-voxel cubes on a 16 x 16 x 16 grid with spacing 3 (copies: 4096 copies of the cube at the grid's
    origin) and 65 rays: 266 240 (ray, instance) pairs, 4160 counts for the scan, more than the 4096 of a chunk."""
    rng = np.random.default_rng(4096)
    models = [(np.full((1, 1, 1), 0xFF0A0B0C, dtype=np.uint32), None)]
    if copies:
        instances = [identity_at((0, 0, 0), (1, 1, 1), 0, FILL) for _ in range(4096)]
    else:
        instances = [identity_at((3 * x, 3 * y, 3 * z), (1, 1, 1), 0, FILL) for x in range(16) for y in range(16) for z in range(16)]
    o, d = [], []
    for corner, sign in (((0, 0, 0), 1), ((15, 15, 15), -1)):  # along the rows that begin in the first and end in the last instance
        for a in range(3):
            start = [3 * v + 0.5 for v in corner]
            start[a] -= 7.5 * sign
            step = [0.0, 0.0, 0.0]
            step[a] = float(sign)
            o.append(start)
            d.append(step)
    for sign in (1.0, -1.0):  # the grid's long diagonal, through 16 cubes' corners ... and beside them
        o.append([0.5 - 4 * sign + (0 if sign > 0 else 45)] * 3)
        d.append([sign] * 3)
    o.append([0.5, 0.5, -5.0])  # at the origin's cube from -z: in both calls a hit
    d.append([0.0, 0.0, 1.0])
    while len(o) < GRID_RAYS:  # from outside at the centre of a random cube
        target = 3 * rng.integers(0, 16, size=3) + rng.uniform(0.2, 0.8, size=3)
        start = rng.uniform(-10, 58, size=3)
        start[rng.integers(0, 3)] = rng.choice([-12.0, 60.0])
        o.append(start)
        d.append(target - start)
    return models, instances, rays_of(o, d, 1e4)


def assert_cube_grid(case, hits, jobs, copies):
    models, instances, rays = case
    pairs = len(rays) * len(instances)
    counts = -(-pairs // WAVE)
    assert len(instances) == 4096 and len(rays) == GRID_RAYS and pairs == 266240 and counts == 4160 > SCAN_CHUNK, "two chunks of the scan"
    hit = hits["instance"][hits["instance"] >= 0]
    if copies:
        assert len(hit) >= 3 and (hit == 0).all() and jobs == 4096 * len(hit), "every hit names instance 0, and every ray that hits has 4096 jobs"
    else:
        assert len(hit) > 30 and hit.min() < 64 and hit.max() > 4031 and len(set(hit.tolist())) > 20 and jobs > 2 * len(rays)


# ---- B4. pick: boxes at +-2^30 --------------------------------------------------------------------------------------------------------------------

def limit_pick_cases():
    """[(name, models, instances, rays, by hand)]: the 4 x 4 x 4 cube with its box ending at +2^30 or beginning at -2^30 on one axis (at 10 .. 14 on
    the other two), and in the corner (-2^30, -2^30, -2^30).  Every origin is exact in float32: on the limit's axis a multiple of 128 voxels from
    the limit (or on it), on the other axes on the cube's half-voxel grid.  Rays along each axis in both directions and along diagonals with
    power-of-two components.  by hand: per ray None (not asserted by hand), "miss", or (voxel, face, model voxel, t)."""
    cases = []
    for ends in (True, False):
        for axis in range(3):
            at = [10, 10, 10]
            at[axis] = LIMIT - 4 if ends else -LIMIT
            b, c = [a for a in range(3) if a != axis]
            o, d, hand = [], [], []

            def ray(origin, direction, expect):
                o.append(origin)
                d.append(direction)
                hand.append(expect)

            def vec(on_axis, on_b, on_c):
                v = [0.0, 0.0, 0.0]
                v[axis], v[b], v[c] = on_axis, on_b, on_c
                return v
            for k in (1, 3):  # along the limit's axis, from 128 k voxels before and behind the limit
                for sign in (1, -1):
                    start = (LIMIT if ends else -LIMIT) - sign * 128 * k
                    first = at[axis] if sign > 0 else at[axis] + 3  # the voxel the ray meets, and the plane it crosses into it
                    plane = first if sign > 0 else first + 1
                    voxel = vec(first, 11, 12)
                    ray(vec(start, 11.5, 12.5), vec(sign, 0, 0), ([int(v) for v in voxel], 2 * axis + (0 if sign > 0 else 1), [int(voxel[a] - at[a]) for a in range(3)], float(abs(plane - start))))
            edge = LIMIT if ends else -LIMIT  # along the other axes, on the limit's plane: +2^30 lies outside the box, -2^30 is its first layer
            for along, other in ((b, c), (c, b)):
                for sign in (1, -1):
                    origin, direction = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
                    origin[axis], origin[along], origin[other] = edge, 12 - 7 * sign, 11.5
                    direction[along] = sign
                    if ends:
                        expect = "miss"
                    else:
                        voxel = [0, 0, 0]
                        voxel[axis], voxel[along], voxel[other] = -LIMIT, 10 if sign > 0 else 13, 11
                        expect = (voxel, 2 * along + (0 if sign > 0 else 1), [voxel[a] - at[a] for a in range(3)], 5.0)
                    ray(origin, direction, expect)
            for sign in (1, -1):  # diagonals with power-of-two components, from 128 voxels before the limit to the cube's middle plane
                for slope in (0.5, -0.25, 1.0):
                    middle = at[axis] + 2
                    start = edge - sign * 128
                    run = abs(middle - start)  # (126 or 130)
                    ray(vec(start, 12 - slope * run, 12.5 + 0.25 * run), vec(sign, slope, -0.25), None)
            cases.append((f"{'ends at +2^30' if ends else 'begins at -2^30'} on axis {axis}", [cube_model()], [identity_at(at, CUBE, 0, FILL)], rays_of(o, d, 1e4), hand))
    at = [-LIMIT] * 3
    o, d = [], []
    for axis in range(3):
        for sign in (1, -1):
            origin, direction = [float(-LIMIT)] * 3, [0.0, 0.0, 0.0]
            origin[axis] = -LIMIT - sign * 128
            direction[axis] = sign
            o.append(origin)
            d.append(direction)
    for direction in ((1, 1, 1), (-1, -1, -1), (1, 0.5, 0.25), (0.5, 1, 0), (-2, -1, -0.5)):
        o.append([-LIMIT + 2 - 130 * v if v > 0 else -LIMIT + 2 - 126 * v for v in direction])
        d.append(direction)
    cases.append(("the corner at -2^30", [cube_model()], [identity_at(at, CUBE, 0, FILL)], rays_of(o, d, 1e4), [None] * len(o)))
    return cases


def assert_limit_pick(case, hits):
    name, models, instances, rays, hand = case
    inst = instances[0]
    lo, hi = np.array(list(inst.boxMin), dtype=np.int64), np.array(list(inst.boxMax), dtype=np.int64)
    assert ((hi == LIMIT) | (lo == -LIMIT)).any() and (hi <= LIMIT).all() and (lo >= -LIMIT).all(), name
    assert (rays["origin"].astype(np.float64) * 2 == np.round(rays["origin"].astype(np.float64) * 2)).all() or "corner" in name, "origins on the half-voxel grid"
    assert (hits["instance"] >= 0).sum() >= 4, name
    for i, expect in enumerate(hand):
        h = hits[i]
        if expect == "miss":
            assert h["instance"] == -1 and h["face"] == -1 and h["voxel"].tolist() == [-1, -1, -1], (name, i, h)
        elif expect is not None:
            voxel, face, model_voxel, t = expect
            assert h["voxel"].tolist() == list(voxel) and h["face"] == face and h["modelVoxel"].tolist() == list(model_voxel) and h["t"] == np.float32(t) and h["instance"] == 0, (name, i, h, expect)
            assert h["argb"] == cube_model()[0][model_voxel[0], model_voxel[2], model_voxel[1]], (name, i)


# ---- A2. the random calls of tests/test_model_contacts_cpu.py ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_pair_calls():
    """[((models, instances, pairs), the model's answer)] of the CPU test's 160 random calls (its own builder; it asserts what they cover)."""
    from test_model_contacts_cpu import random_calls
    return [(case[:3], model_of(*case[:3])) for case in random_calls()]


# ---- C. the flight loop: carve, lift, test poses, pick, place -------------------------------------------------------------------------------------

FLIGHT_DIMS = (64, 64, 64)
FLIGHT_LEVELS = 5  # LOD 1 .. 5 are rebuilt by every edit
GROUND, NECK = 8, (24, 28)
SOLID_OUTSIDE = gpu.SURFACE_OUTSIDE_DEFAULT


@functools.lru_cache(maxsize=None)
def flight_world():
    """(solid, colour, the carve stroke, the pieces): ground below y = 8 with three pillars whose heads differ in shape -- a notched slab, a stepped
    pyramid, a ball --; the stroke cuts the three necks at y in [24, 28).  The pieces are what floats then, by name: (min, size, argb, mask) with
    the arrays (X, Z, Y) over the piece's box, as cvx_world_lift_pieces stores them.  The volumes are those BEFORE the stroke."""
    from scipy import ndimage
    import pickmodel
    solid = np.zeros(FLIGHT_DIMS, dtype=bool)
    solid[:, :GROUND, :] = True
    solid[10:14, GROUND:30, 12:16] = True  # "slab"
    solid[8:15, 30:33, 11:16] = True
    solid[8:10, 30:33, 11:13] = False
    solid[30:34, GROUND:30, 30:34] = True  # "pyramid"
    for k in range(6):
        solid[26 + k:38 - k, 30 + k, 26 + k:38 - k] = True
    solid[48:52, GROUND:32, 14:18] = True  # "ball"
    x, y, z = np.meshgrid(*[np.arange(n) + 0.5 for n in FLIGHT_DIMS], indexing="ij")
    solid |= (x - 50.5) ** 2 + (y - 35.5) ** 2 + (z - 16.5) ** 2 <= 5.4 ** 2
    colour = np.where(solid, np.uint32(0xFF000000) | (np.arange(64, dtype=np.uint32)[:, None, None] << 16) | (np.arange(64, dtype=np.uint32)[None, :, None] << 8) |
                      np.arange(64, dtype=np.uint32)[None, None, :], 0).astype(np.uint32)
    neck = [{"op": gpu.BRUSH_CARVE, "shape": 0, "a": (0, NECK[0], 0), "b": (FLIGHT_DIMS[0], NECK[1], FLIGHT_DIMS[2]), "argb": 0}]
    cut_solid, cut_colour = solid.copy(), colour.copy()
    pickmodel.apply_strokes(cut_solid, cut_colour, neck)
    labels, count = ndimage.label(cut_solid, structure=ndimage.generate_binary_structure(3, 1))
    pieces = {}
    for name, inside in (("slab", (11, 31, 13)), ("pyramid", (32, 31, 32)), ("ball", (50, 35, 16))):
        mine = labels == labels[inside]
        where = np.nonzero(mine)
        lo = [int(w.min()) for w in where]
        hi = [int(w.max()) + 1 for w in where]
        box = tuple(slice(lo[a], hi[a]) for a in range(3))
        pieces[name] = (lo, [hi[a] - lo[a] for a in range(3)], np.ascontiguousarray(np.where(mine[box], cut_colour[box], 0).transpose(0, 2, 1)),
                        np.ascontiguousarray(mine[box].transpose(0, 2, 1)))
    assert count == 4 and not labels[inside] == labels[0, 0, 0]
    return solid, colour, neck, pieces


def flight_after_lift():
    """The world's volumes after the stroke and the LIFT_REMOVE of the three pieces: the ground and the three stumps."""
    import pickmodel
    solid, colour, neck, pieces = flight_world()
    solid, colour = solid.copy(), colour.copy()
    pickmodel.apply_strokes(solid, colour, neck)
    solid[:, NECK[1]:, :] = False
    colour[~solid] = 0
    return solid, colour


FLIGHT_POSES = (  # (name, piece, how, where): "at" the corner of an identity move, "quarter" / "tilt" the centre of the turned body
    ("slab where it was", "slab", "at", None), ("slab in the ground", "slab", "at", (20, 7, 40)), ("pyramid two layers in the ground", "pyramid", "at", (40, 6, 44)),
    ("ball turned, in the ground", "ball", "quarter", (20.5, 13.5, 52.5)), ("slab on its stump", "slab", "at", (8, 23, 11)), ("pyramid on the ball's stump", "pyramid", "at", (44, 22, 10)),
    ("slab tilted in the air", "slab", "tilt", (20.0, 44.0, 20.0)), ("ball tilted on the pyramid's stump", "ball", "tilt", (32.0, 28.5, 32.0)),
    ("pyramid in the air", "pyramid", "at", (6, 40, 36)), ("slab inside the pyramid", "slab", "at", (9, 41, 40)), ("ball through the tilted slab", "ball", "at", (17, 40, 15)),
    ("slab below a slab", "slab", "at", (40, 30, 50)), ("slab a layer into the one below", "slab", "at", (42, 34, 50)), ("pyramid high up", "pyramid", "at", (46, 52, 46)),
    ("ball high up", "ball", "at", (5, 50, 4)))


def flight_instances(order):
    """The poses as instances; `order`: the pieces' names in the order of the models (the device's order of the lifted pieces)."""
    pieces = flight_world()[3]
    out = []
    for name, piece, how, where in FLIGHT_POSES:
        lo, size = pieces[piece][:2]
        model = list(order).index(piece)
        if how == "at":
            out.append(identity_at(lo if where is None else where, size, model, FILL))
        else:
            out.append(gpu.model_instance(forward_about_centre(rotation(1, 90) if how == "quarter" else tilt(), size, where), size, model, FILL))
    return out


def flight_rays():
    """A grid of 16 x 16 rays from above, a little off the vertical, and 256 of pickmodel's random rays."""
    import pickmodel
    rng = np.random.default_rng(707)
    gx, gz = np.meshgrid(np.arange(16) * 4.0 + 1.37, np.arange(16) * 4.0 + 2.21, indexing="ij")
    o = np.stack([gx.ravel(), np.full(256, 70.0), gz.ravel()], axis=-1)
    d = np.tile(np.array([0.03, -1.0, 0.02]), (256, 1))
    o2, d2, t2 = pickmodel.random_rays(rng, FLIGHT_DIMS, 256)
    boxes = np.array([[list(i.boxMin), list(i.boxMax)] for i in flight_instances(("slab", "pyramid", "ball"))], dtype=np.float64)  # (the boxes do not depend on the order)
    aimed = np.arange(256) % 4 != 0  # three in four of them at a random point of a pose's box
    which = rng.integers(0, len(boxes), size=256)
    target = boxes[which, 0] + rng.uniform(0.0, 1.0, size=(256, 3)) * (boxes[which, 1] - boxes[which, 0])
    d2[aimed] = (target - o2)[aimed]
    t2[aimed] = 1e4
    return rays_of(np.concatenate([o, o2]), np.concatenate([d, d2]), np.concatenate([np.full(256, 1e4), t2]))


def assert_flight_poses(world_answer, pair_answer, pairs):
    """From the models' answers (tests/contactsmodel.py over the world after the lift, tests/paircontactsmodel.py over gpu.box_pairs): -> the free poses."""
    names = [p[0] for p in FLIGHT_POSES]
    results = world_answer[0]
    met = results["overlap"] > 0
    in_ground = met & (results["max"][:, 1] <= GROUND)
    on_stump = met & (results["min"][:, 1] >= GROUND)
    assert in_ground.sum() >= 3 and on_stump.sum() >= 3, (in_ground.tolist(), on_stump.tolist())
    assert in_ground[names.index("ball turned, in the ground")] and on_stump[names.index("ball tilted on the pyramid's stump")] and on_stump[names.index("slab on its stump")]
    pair_results = pair_answer[0]
    touching = pair_results["overlap"] > 0
    assert touching.sum() >= 3, "two pairs of bodies overlap, and one more touches"
    layer = touching & ((pair_results["max"] - pair_results["min"]) == 1).any(axis=1)
    deep = touching & ((pair_results["max"] - pair_results["min"]) > 1).all(axis=1)
    assert layer.sum() >= 1 and deep.sum() >= 2, "one pair touches in a single layer, two overlap"
    in_pair = np.zeros(len(names), dtype=bool)
    in_pair[np.asarray(pairs)[touching].ravel()] = True
    free = ~met & ~in_pair
    assert free.sum() >= 3 and free[names.index("slab where it was")] and free[names.index("pyramid high up")] and free[names.index("ball high up")], free.tolist()
    return np.nonzero(free)[0]
