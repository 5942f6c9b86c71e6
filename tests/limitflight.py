"""Test infrastructure (numpy only, no device): the calls of tests/test_gpu_flight_kernel_limits.py and tests/test_gpu_flight_sequences.py, the calls for
bodies in flight (cvxs_world_sweep, cvxm_pair_sweep, cvxd_models_brush) at their kernels' compiled limits, TOGETHER with the counts and
properties each case is named after, computed from the numpy models (tests/sweepmodel.py, tests/pairsweepmodel.py, tests/modelbrushmodel.py),
sweepmodel.jobs / pairsweepmodel.pair_jobs or plain prefix arithmetic (tests/test_limit_flight_cpu.py checks them on the CPU and runs every call
through the host rules programs; the GPU tests repeat the cheap ones before they call the device).

The limits are constants of the .hip files: the 65536 workgroups of a launch (2^18 waves: beyond them the waves take the jobs in turn), the 64
strokes of a list word, the 1024 elements of an apply chunk and the 64 of its steps, the 32 bits a coordinate product, a wave's sum and a
model's sum must not be cut to, the first probe step of 1024 of the pair search, and +-2^30, the last coordinate the validation lets through.

A pair's answer depends on (a, b, v) alone and a body's brush answer on its own model and the strokes that reach it, so the large calls are
tiled from a few distinct units; tests/test_limit_flight_cpu.py checks each tiling helper against the model on a call small enough for it."""
from __future__ import annotations

import functools

import numpy as np

import limitmodels as L
import modelbrushcases
import modelbrushmodel
import paircontactsmodel
import pairsweepcases
import pairsweepmodel
import sweepcases
import sweepmodel
from cpuvox_amd import gpu
from modelbrushcases import CARVE, PAINT, box, capsule, ellipsoid, sphere
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, random_model, rotation

LIMIT = L.LIMIT
TURN = 1 << 18        # the waves of a launch of kMaxWorkgroups = 65536 workgroups: job TURN is the first a wave takes as its second
CHUNK = 1024          # cvxb::kModelBrushChunk
MAX_T = 1 << 46       # cvxb::kModelMapMaxT, in units of 2^-16
FILL = gpu.BRUSH_FILL
DEFAULT = gpu.SURFACE_OUTSIDE_DEFAULT


def boxes_of(instances):
    return (np.array([list(i.boxMin) for i in instances], dtype=np.int64), np.array([list(i.boxMax) for i in instances], dtype=np.int64))


# ---- A1. world sweep: more than 2^18 jobs ------------------------------------------------------------------------------------------------------------

SWEEP_BODIES, SWEEP_UNITS, SWEEP_SIZE, SWEEP_STATIONS = 72, 24, (8, 3, 8), 60


@functools.lru_cache(maxsize=None)
def many_stations(reverse=False):
    """(world key, models, instances, motions, solid_outside): 72 bodies with a footprint of 8 x 8 over the terrain, 24 distinct (place, motion)
    in turn, every motion with |vx| + |vz| = 59: 60 stations, 3840 jobs a body, 276 480 in all.  Every body starts a few voxels above the terrain
    below it and comes down across it.  reverse: the same call with the list reversed."""
    rng = np.random.default_rng(2618)
    _, solid, colour = sweepcases.world("terrain")
    models = [random_model(np.random.default_rng(2619), SWEEP_SIZE, zeros=0.3)]
    units = []
    while len(units) < SWEEP_UNITS:  # drawn until the model says the body flies 16 stations or more before it touches
        u = len(units)
        vx = int(rng.integers(20, 40)) * (1 if u % 2 else -1)
        vz = (SWEEP_STATIONS - 1 - abs(vx)) * (1 if u % 4 < 2 else -1)
        x, z = (70 if vx < 0 else 10) + int(rng.integers(0, 40)), (70 if vz < 0 else 10) + int(rng.integers(0, 40))
        y = int(np.nonzero(solid[x:x + 8, :, z:z + 8].any(axis=(0, 2)))[0].max()) + 2 + int(rng.integers(0, 6))
        v = (vx, -int(rng.integers(4, 30)), vz)
        hit, _ = sweepmodel._one(solid, colour, models, as_dicts([identity_at((x, y, z), SWEEP_SIZE, 0, FILL)])[0], v, DEFAULT)
        if hit > 0 and station_of(v, hit) >= 16:
            units.append(((x, y, z), v))
    order = [k % SWEEP_UNITS for k in range(SWEEP_BODIES)]
    if reverse:
        order = order[::-1]
    return "terrain", models, [identity_at(units[u][0], SWEEP_SIZE, 0, FILL) for u in order], [units[u][1] for u in order], DEFAULT


@functools.lru_cache(maxsize=None)
def sweep_answer(reverse=False):
    key, models, instances, motions, so = many_stations(reverse)
    return world_sweep_model(key, models, instances, motions, so)


def world_sweep_model(key, models, instances, motions, so):
    _, solid, colour = sweepcases.world(key)
    return world_sweep_model_on(solid, colour, models, instances, motions, so)


def world_sweep_model_on(solid, colour, models, instances, motions, so):
    """sweepmodel.sweep with the summary's jobs: (sweeps, contacts, points, summary)."""
    dicts = as_dicts(instances)
    sweeps, contacts, points, summary = sweepmodel.sweep(solid, colour, models, dicts, motions, so)
    summary["jobs"] = sweepmodel.jobs(dicts, motions)
    return sweeps, contacts, points, summary


def station_of(motion, j):
    """The station pose j of the motion's path belongs to: the horizontal steps among its first j (the model's path, counted)."""
    return sum(1 for _, axis in sweepmodel.path(motion)[1:j + 1] if axis != 1)


def sweep_prefix(instances, motions):
    """The jobs before every instance, and all of them last: footprint * stations, from sweepmodel.jobs an instance at a time."""
    dicts = as_dicts(instances)
    return np.concatenate([[0], np.cumsum([sweepmodel.jobs([d], [v]) for d, v in zip(dicts, motions)])])


def assert_many_stations():
    key, models, instances, motions, so = many_stations()
    sweeps, contacts, points, summary = sweep_answer()
    prefix = sweep_prefix(instances, motions)
    assert len(instances) == SWEEP_BODIES and (np.diff(prefix) == 64 * SWEEP_STATIONS).all() and prefix[-1] == summary["jobs"] == 276480 > TURN
    assert all(abs(v[0]) + abs(v[2]) == SWEEP_STATIONS - 1 for v in motions)
    beyond = np.nonzero(prefix[:-1] >= TURN)[0]
    assert len(beyond) >= 3 and (sweeps["hit"][beyond] > 0).all(), "bodies whose every job is a wave's second, and they hit on the way"
    straddling = np.nonzero((prefix[:-1] < TURN) & (prefix[1:] > TURN))[0]
    assert len(straddling) == 1
    k = int(straddling[0])
    hit = int(sweeps["hit"][k])
    assert hit > 0 and prefix[k] + 64 * station_of(motions[k], hit) >= TURN, "the straddling body hits in a station whose jobs lie past 2^18"
    assert (sweeps["hit"] > 0).all() and {0, 1, 2} <= set(sweeps["axis"][sweeps["hit"] > 0].tolist()) and summary["points"] > 0
    return dict(jobs=int(prefix[-1]), beyond=len(beyond), straddling=k, station=station_of(motions[k], hit))


def assert_reversed_sweep(forward, back):
    """The reversed call's answer is the forward call's per body, but for firstPoint, the list's order."""
    assert back[0][::-1].tobytes() == forward[0].tobytes() and back[3] == forward[3]
    mine, theirs = back[1][::-1].copy(), forward[1].copy()
    mine["firstPoint"] = theirs["firstPoint"] = 0
    assert mine.tobytes() == theirs.tobytes() and (back[1]["firstPoint"][::-1] != forward[1]["firstPoint"]).any()


# ---- B. pair sweep: more than 2^18 jobs, and runs of pairs without jobs -----------------------------------------------------------------------------

PAIR_SIZE, SMALL_SIZE = (8, 2, 8), (2, 2, 2)
MANY_PAIRS, LAST_PAIRS = 4200, 100


@functools.lru_cache(maxsize=None)
def pair_units(size=PAIR_SIZE):
    """(models, instances, unit pairs, unit motions, D, the model's answer for the units): a sparse random body a of `size` above a body b as it
    lies, above a b turned by 30 degrees about y and upon a copy of itself; the first D units have every column of a as a job (the footprints
    coincide and the motion brings a down into b's layers), among them motions that hit on the way, motions that pass between b's voxels and one
    pair that starts overlapping; the last two lead away and have no job."""
    rng = np.random.default_rng(418 + size[0])
    zeros = 0.92 if size[0] > 2 else 0.45
    models = [random_model(rng, size, zeros=zeros), random_model(rng, size, with_mask=True, zeros=zeros)]
    centre = np.array([size[0] / 2, 2 + size[1] / 2, size[2] / 2])
    instances = [identity_at((0, 10, 0), size, 0, FILL), identity_at((0, 2, 0), size, 1, FILL),
                 gpu.model_instance(forward_about_centre(rotation(1, 30), size, centre), size, 1, FILL), identity_at((0, 10, 0), size, 0, FILL)]
    pairs, motions = [], []
    for b in (1, 2):
        for v in ((0, -12, 0), (1, -7, -1), (-2, -8, 1), (0, -7, 0), (2, -9, 2), (-1, -10, -2), (3, -7, 2), (-3, -7, -3)):
            pairs.append((0, b))
            motions.append(v)
    pairs.append((0, 3))
    motions.append((0, -9, 1))
    d = len(pairs)
    pairs += [(0, 1), (0, 2)]
    motions += [(0, 5, 0), (1, 3, 0)]
    answer = pairsweepmodel.sweep(models, as_dicts(instances), pairs, motions)
    return models, instances, np.int32(pairs), np.int32(motions), d, answer


def unit_jobs(size=PAIR_SIZE):
    models, instances, pairs, motions, d, _ = pair_units(size)
    dicts = as_dicts(instances)
    return np.array([pairsweepmodel.pair_jobs(dicts[int(a)], dicts[int(b)], v) for (a, b), v in zip(pairs, motions)], dtype=np.int64)


def tile_sweeps(base_answer, base_jobs, which):
    """The model's answer of the call whose pair p is unit which[p]: sweeps and contacts gathered, firstPoint the running sum of the points
    before, the summary added up."""
    sweeps, contacts, _ = base_answer
    which = np.asarray(which)
    tiled, results = sweeps[which].copy(), contacts[which].copy()
    counts = results["points"].astype(np.int64)
    results["firstPoint"] = np.cumsum(counts) - counts
    hit = tiled["sweep"]["hit"]
    return tiled, results, dict(hits=int((hit >= 0).sum()), startsSolid=int((hit == 0).sum()), jobs=int(np.asarray(base_jobs)[which].sum()))


def tiled_pair_call(which, size=PAIR_SIZE):
    """(models, instances, pairs, motions, the tiled answer) of the call whose pair p is unit which[p]."""
    models, instances, pairs, motions, _, answer = pair_units(size)
    return models, instances, np.ascontiguousarray(pairs[which]), np.ascontiguousarray(motions[which]), tile_sweeps(answer, unit_jobs(size), which)


@functools.lru_cache(maxsize=None)
def many_pair_jobs():
    """B1: 4200 pairs of the 8 x 2 x 8 units in turn: 64 jobs each, 268 800 in all."""
    return tiled_pair_call(np.arange(MANY_PAIRS) % pair_units()[4])


@functools.lru_cache(maxsize=None)
def pair_empty_runs():
    """B2: 65536 pairs of the 2 x 2 x 2 units in turn, with limitmodels.empty_runs' three runs of 1100 pairs without jobs."""
    d = pair_units(SMALL_SIZE)[4]
    which = np.arange(65536) % d
    for lo, hi in L.empty_runs(65536):
        which[lo:hi] = d + np.arange(hi - lo) % 2
    return tiled_pair_call(which, SMALL_SIZE)


def assert_pair_units(size=PAIR_SIZE):
    models, instances, pairs, motions, d, (sweeps, contacts, summary) = pair_units(size)
    jobs = unit_jobs(size)
    assert d >= 8 and len({(int(a), int(b), tuple(v.tolist())) for (a, b), v in zip(pairs[:d], motions[:d])}) == d, "at least 8 distinct (a, b, v)"
    assert (jobs[:d] == size[0] * size[2]).all() and (jobs[d:] == 0).all() and len(jobs) == d + 2, "every column of a is a job; the last two units have none"
    hit = sweeps["sweep"]["hit"]
    assert (hit[:d] > 0).sum() >= 3 and (hit[:d] == -1).sum() >= 2 and (hit[:d] == 0).sum() == 1 and (hit[d:] == -1).all(), hit.tolist()
    lo, hi = boxes_of(instances)
    assert (hi[2] - lo[2])[[0, 2]].min() > size[0], "the turned body's box is wider than the body"


def assert_many_pair_jobs():
    models, instances, pairs, motions, (sweeps, contacts, summary) = many_pair_jobs()
    prefix = np.concatenate([[0], np.cumsum(pairsweep_jobs(instances, pairs, motions))])
    assert len(pairs) == MANY_PAIRS and (np.diff(prefix) == 64).all() and prefix[-1] == summary["jobs"] == 268800 > TURN
    last = sweeps["sweep"]["hit"][-LAST_PAIRS:]
    assert prefix[MANY_PAIRS - LAST_PAIRS] >= TURN, "the last 100 pairs lie wholly past job 2^18"
    assert (last > 0).sum() >= 20 and (last == -1).sum() >= 10 and (last == 0).sum() >= 1, "hits on the way, misses and a pair that starts overlapping among them"
    return dict(jobs=int(prefix[-1]), pairs=len(pairs))


def pairsweep_jobs(instances, pairs, motions):
    """Per pair its jobs by pairsweepmodel.pair_jobs, one computation per distinct (a, b, v)."""
    dicts = as_dicts(instances)
    seen = {}
    out = np.zeros(len(pairs), dtype=np.int64)
    for p, ((a, b), v) in enumerate(zip(np.asarray(pairs).tolist(), np.asarray(motions).tolist())):
        key = (a, b, tuple(v))
        if key not in seen:
            seen[key] = pairsweepmodel.pair_jobs(dicts[a], dicts[b], v)
        out[p] = seen[key]
    return out


def assert_pair_empty_runs():
    models, instances, pairs, motions, (sweeps, contacts, summary) = pair_empty_runs()
    runs = L.empty_runs(65536)
    prefix = np.concatenate([[0], np.cumsum(pairsweep_jobs(instances, pairs, motions))])
    assert len(pairs) == 65536 and len(runs) == 3 and prefix[-1] == summary["jobs"]
    in_run = np.zeros(65536, dtype=bool)
    for lo, hi in runs:
        in_run[lo:hi] = True
        assert hi - lo >= L.RUN_LENGTH > L.PROBE_STEP and (prefix[lo:hi + 1] == prefix[lo]).all() and (sweeps["sweep"]["hit"][lo:hi] == -1).all(), "the prefix is flat over a run"
    assert runs[0][0] == 0 and runs[2][1] == 65536 and runs[1][0] // L.PROBE_STEP < (runs[1][1] - 1) // L.PROBE_STEP
    assert (np.diff(prefix)[~in_run] > 0).all() and (sweeps["sweep"]["hit"][~in_run] > 0).sum() > 10000, "the prefix grows elsewhere, and pairs there hit"
    return dict(jobs=int(prefix[-1]), pairs=len(pairs))


# ---- C. the model brush ------------------------------------------------------------------------------------------------------------------------------

def footprints(strokes):
    """The strokes' footprint boxes (lo, hi), two integer arrays of shape (strokes, 3): the model's own."""
    boxes = [modelbrushmodel._footprint(s) for s in strokes]
    return np.array([b[0] for b in boxes], dtype=np.int64), np.array([b[1] for b in boxes], dtype=np.int64)


def reaches(instances, strokes):
    """reaches[k, j]: stroke j's footprint meets instance k's box on all three axes (plain arithmetic): the cull's bit j of instance k."""
    lo, hi = boxes_of(instances)
    s_lo, s_hi = footprints(strokes)
    return ((s_lo[None, :, :] < hi[:, None, :]) & (s_hi[None, :, :] > lo[:, None, :])).all(axis=2)


def brush_by_body(models, instances, strokes):
    """modelbrushmodel.brush of a call in which every instance has a model of its own, a body at a time with the strokes that reach it alone: a
    stroke whose footprint misses a body's box holds at none of its voxels (the model's own first test), and what is left keeps its order.  The
    colours are the strokes', not their indices: the answer is the whole call's."""
    assert [i.model for i in instances] == list(range(len(models)))
    reach = reaches(instances, strokes)
    dicts = as_dicts(instances)
    after, results, hit = [], np.zeros(len(models), dtype=modelbrushmodel.RESULT_DTYPE), np.zeros(len(instances), dtype=modelbrushmodel.INSTANCE_DTYPE)
    for k, (model, inst) in enumerate(zip(models, dicts)):
        mine = [strokes[j] for j in np.nonzero(reach[k])[0]] or [strokes[0]]
        a, r, h, _ = modelbrushmodel.brush([model], [dict(inst, model=0)], mine)
        after.append(a[0])
        results[k], hit[k] = r[0], h[0]
    summary = dict(carved=int(results["carved"].sum()), painted=int(results["painted"].sum()), models=int(((results["carved"] + results["painted"]) > 0).sum()),
                   jobs=modelbrushmodel.jobs(dicts, strokes))
    return after, results, hit, summary


def brush_model(models, instances, strokes):
    return modelbrushmodel.brush(models, as_dicts(instances), strokes)


# C1. more than 2^18 mark jobs

MARK_BODIES, MARK_SIZE, MARK_LAST = 300, (30, 2, 30), range(292, 300)


@functools.lru_cache(maxsize=None)
def many_mark_jobs():
    """(models, instances, strokes): 300 bodies of 30 x 2 x 30 over three models -- a mask alone, colours alone, both --, on a grid 40 apart.  One
    PAINT box over the lower layer of them all; then eight strokes of every shape, each on one of bodies 292 .. 299 alone."""
    rng = np.random.default_rng(300)
    both = [random_model(rng, MARK_SIZE, with_mask=True, zeros=0.3) for _ in range(3)]
    models = [(None, np.array(both[0][1])), (np.where(both[1][1], both[1][0] | 0xFF000000, 0).astype(np.uint32), None), both[2]]
    at = lambda k: (40 * (k % 20), 0, 40 * (k // 20))  # noqa: E731
    instances = [identity_at(at(k), MARK_SIZE, k % 3, FILL) for k in range(MARK_BODIES)]
    strokes = [box(PAINT, (-5, 0, -5), (805, 1, 605), 0xFF123456)]
    for n, k in enumerate(MARK_LAST):
        x, _, z = at(k)
        c = (x + 8 + 2 * n, 1, z + 20 - n)
        strokes.append([sphere(CARVE, c, 3 + n), capsule(CARVE, c, (c[0] + 9, 0, c[2] + n), 1), ellipsoid(CARVE, c, (4 + n, 2, 11 - n)), box(CARVE, c, (c[0] + 1 + n, 2, c[2] + 7))][n % 4])
    return models, instances, strokes


@functools.lru_cache(maxsize=None)
def mark_answer():
    return brush_model(*many_mark_jobs())


def brush_prefix(instances, strokes):
    """The mark jobs before every instance, and all of them last: modelbrushmodel.jobs an instance at a time (the reach is the whole call's)."""
    dicts = as_dicts(instances)
    boxes = [modelbrushmodel._footprint(s) for s in strokes]
    around = [box(CARVE, [min(b[0][i] for b in boxes) for i in range(3)], [max(b[1][i] for b in boxes) for i in range(3)])]
    return np.concatenate([[0], np.cumsum([modelbrushmodel.jobs([d], around) for d in dicts])])


def assert_many_mark_jobs():
    models, instances, strokes = many_mark_jobs()
    after, results, hit, summary = mark_answer()
    prefix = brush_prefix(instances, strokes)
    assert len(instances) == MARK_BODIES and (np.diff(prefix) == 900).all() and prefix[-1] == summary["jobs"] == 270000 > TURN
    assert prefix[MARK_LAST[0]] >= TURN, "every job of bodies 292 .. 299 is a wave's second"
    reach = reaches(instances, strokes)
    assert reach[:, 0].all() and (reach[:, 1:].sum(axis=0) == 1).all() and [int(np.nonzero(reach[:, 1 + n])[0][0]) for n in range(8)] == list(MARK_LAST)
    last = hit[list(MARK_LAST)]
    assert (last["carved"] > 0).all() and len({(int(c), int(p)) for c, p in last.tolist()}) == 8, last.tolist()
    assert (hit["painted"][1::3] > 0).all() and (hit["painted"][2::3] > 0).all() and not hit["painted"][0::3].any(), "a mask alone takes no PAINT"
    assert summary["models"] == 3
    return dict(jobs=int(prefix[-1]))


# C2. list rows

ROW_STROKES, ROW_BODIES = (65, 128, 129, 4096), (5, 65)
ROW_COLOUR = 0xFF100000


@functools.lru_cache(maxsize=None)
def list_rows(stroke_count, body_count):
    """(models, instances, strokes): `body_count` bodies of 4 x 4 x 4 far apart, each with a ramp model of its own (every third with a mask too),
    under `stroke_count` strokes of one voxel each.  Body k >= 1 is reached by PAINT k - 1 (list word 0), by PAINT 64 (words - 1) + k - 1 (the last
    word; where the list is that long: the last word of 65 and of 129 strokes holds one stroke) and, where there are words between the two, by
    one CARVE in one of them; none of these reaches another body.  Every other stroke lands on body 0, four in five a PAINT.  PAINT j has the
    colour 0xFF100000 + j."""
    words = -(-stroke_count // 64)
    size = (4, 4, 4)
    models = []
    for k in range(body_count):
        argb = modelbrushcases._ramp(size)[0] + np.uint32(0x1000 * k)
        models.append((argb, np.ones(argb.shape, dtype=bool)) if k % 3 == 2 else (argb, None))
    at = lambda k: (100 * k - 3000, 7 * (k % 5), 11 * (k % 7) - 30)  # noqa: E731
    instances = [identity_at(at(k), size, k, FILL) for k in range(body_count)]
    strokes = [None] * stroke_count
    voxel = lambda k, v: tuple(int(at(k)[a]) + v[a] for a in range(3))  # noqa: E731
    for k in range(1, body_count):
        strokes[k - 1] = sphere(PAINT, voxel(k, (0, k % 4, 1)), 0, ROW_COLOUR + k - 1)
        j = 64 * (words - 1) + k - 1
        if j < stroke_count:
            strokes[j] = sphere(PAINT, voxel(k, (3, 3, k % 4)), 0, ROW_COLOUR + j)
        if words > 2:
            j = 64 * (1 + (k - 1) % (words - 2)) + (k - 1) // (words - 2)
            strokes[j] = sphere(CARVE, voxel(k, (2, 1, 2)), 0)
    for j in range(stroke_count):
        if strokes[j] is None:
            v = (j * 7) % 64
            strokes[j] = sphere(CARVE if j % 5 == 4 else PAINT, voxel(0, (v // 16, v // 4 % 4, v % 4)), 0, 0 if j % 5 == 4 else ROW_COLOUR + j)
    return models, instances, strokes


@functools.lru_cache(maxsize=None)
def rows_answer(stroke_count, body_count):
    return brush_by_body(*list_rows(stroke_count, body_count))


def assert_list_rows(stroke_count, body_count):
    models, instances, strokes = list_rows(stroke_count, body_count)
    after, results, hit, summary = rows_answer(stroke_count, body_count)
    words = -(-stroke_count // 64)
    reach = reaches(instances, strokes)
    assert reach.shape == (body_count, stroke_count) and (reach.sum(axis=0) == 1).all(), "every stroke reaches one body"
    for w in range(words):
        assert reach[:, 64 * w:64 * w + 64].any(axis=1).sum() >= (2 if w in (0, words - 1) and words > 1 and 64 * w + 1 < stroke_count else 1), f"list word {w} has a set bit"
    assert len({tuple(np.nonzero(row)[0].tolist()) for row in reach}) == body_count, "no two bodies have the same set of strokes"
    in_last = 0
    for k in range(1, body_count):
        mine = np.nonzero(reach[k])[0]
        assert mine[0] == k - 1 < 64 and strokes[k - 1]["op"] == PAINT and (after[k][0] == ROW_COLOUR + k - 1).sum() == 1, "a PAINT of word 0, legible in the array"
        j = 64 * (words - 1) + k - 1
        if j < stroke_count:
            in_last += 1
            assert mine[-1] == j and (after[k][0] == ROW_COLOUR + j).sum() == 1, "a PAINT of the last word"
        assert results[k]["carved"] == (1 if words > 2 else 0) and hit[k]["painted"] == len(mine) - results[k]["carved"], (k, mine.tolist(), results[k], hit[k])
    assert in_last == min(body_count - 1, stroke_count - 64 * (words - 1)) >= 1
    ops = [s["op"] for s in strokes]
    on_first = int(reach[0].sum())  # (65 and 128 strokes on 65 bodies: the bodies' PAINTs are all but one or none of the strokes)
    assert ops.count(PAINT) >= 50 and ops.count(CARVE) >= on_first // 5 and (on_first < 5 or ops.count(CARVE) > 0), "some strokes are CARVEs"
    assert on_first == 0 or results[0]["carved"] + results[0]["painted"] > 0
    return dict(words=words, jobs=summary["jobs"])


# C3. chunk edges

EDGE_SIZES = ((3, 11, 31), (8, 16, 8), (5, 41, 5), (1, 1087, 1), (8, 17, 8), (3, 33, 11), (3, 683, 1), (16, 12, 16))
EDGE_VOLUMES = (1023, 1024, 1025, 1087, 1088, 1089, 2049, 3072)


def _voxel_of(size, at):
    """Element `at` of a model of `size` (laid out (X, Z, Y), y fastest) -> its voxel (x, y, z)."""
    column, y = divmod(at, size[1])
    x, z = divmod(column, size[2])
    return x, y, z


@functools.lru_cache(maxsize=None)
def chunk_edges():
    """(models, instances, strokes, the elements struck per model): eight models whose volumes lie on and either side of a multiple of 1024
    and of 64 inside the last chunk, in one call; a mask alone, colours alone and both in turn, every element set and ramp-coloured.  A stroke
    of one voxel lands on the last element of every model (a CARVE) and on the first element of each later chunk (a PAINT, a CARVE on a mask
    alone)."""
    models, instances, strokes, struck = [], [], [], []
    for g, size in enumerate(EDGE_SIZES):
        argb = modelbrushcases._ramp(size)[0]
        mask = np.ones(argb.shape, dtype=bool)
        models.append([(None, mask), (argb, None), (argb, mask)][g % 3])
        corner = (200 * g - 700, -40 + 13 * g, 5 * g)
        instances.append(identity_at(corner, size, g, FILL))
        volume = size[0] * size[1] * size[2]
        mine = [volume - 1] + [CHUNK * c for c in range(1, -(-volume // CHUNK)) if CHUNK * c != volume - 1]
        struck.append(mine)
        for n, at in enumerate(mine):
            v = _voxel_of(size, at)
            paint = n > 0 and g % 3 != 0
            strokes.append(sphere(PAINT if paint else CARVE, [corner[a] + v[a] for a in range(3)], 0, 0xFF200000 + len(strokes) if paint else 0))
    return models, instances, strokes, struck


@functools.lru_cache(maxsize=None)
def edges_answer():
    return brush_model(*chunk_edges()[:3])


def assert_chunk_edges():
    models, instances, strokes, struck = chunk_edges()
    after, results, hit, summary = edges_answer()
    volumes = [s[0] * s[1] * s[2] for s in EDGE_SIZES]
    assert tuple(volumes) == EDGE_VOLUMES and [-(-v // CHUNK) for v in volumes] == [1, 1, 2, 2, 2, 2, 3, 3]
    assert [(m[0] is not None, m[1] is not None) for m in models[:3]] == [(False, True), (True, False), (True, True)]
    untouched = brush_model(models, instances, [sphere(CARVE, (9000, 9000, 9000), 0)])[1]
    assert (untouched["voxels"] == volumes).all() and not untouched["carved"].any()
    for g, (r, u) in enumerate(zip(results, untouched)):
        assert r["carved"] >= 1 and r["carved"] + r["painted"] == len(struck[g]) and r["voxels"] == volumes[g] - r["carved"], g
        assert b"".join(r[name].tobytes() for name in ("min", "max", "sum", "moment")) != b"".join(u[name].tobytes() for name in ("min", "max", "sum", "moment")), g
        flat = (after[g][1] if models[g][0] is None else after[g][0]).reshape(-1)
        for n, at in enumerate(struck[g]):
            before = True if models[g][0] is None else int(models[g][0].reshape(-1)[at])
            assert flat[at] != before and (n == 0 or at % CHUNK == 0) and (n > 0 or at == volumes[g] - 1), (g, at)
    return dict(chunks=[-(-v // CHUNK) for v in volumes], jobs=summary["jobs"])


# C4. wide sums

WIDE_SIZE = (66000, 2, 3)


@functools.lru_cache(maxsize=None)
def wide_sums():
    """(models, instances, strokes): a 66000 x 2 x 3 model, every voxel set, behind a small one (so that its elements do not begin at 0), its last
    voxel carved.  The small body lies out of the stroke's reach."""
    small = modelbrushcases._ramp((2, 2, 2))
    wide = (None, np.ones((WIDE_SIZE[0], WIDE_SIZE[2], WIDE_SIZE[1]), dtype=bool))
    instances = [identity_at((0, 100, 0), (2, 2, 2), 0, FILL), identity_at((-7, 0, 4), WIDE_SIZE, 1, FILL)]
    return [small, wide], instances, [sphere(CARVE, (-7 + WIDE_SIZE[0] - 1, 1, 4 + 2), 0)]


@functools.lru_cache(maxsize=None)
def wide_answer():
    return brush_model(*wide_sums())


def assert_wide_sums():
    models, instances, strokes = wide_sums()
    after, results, hit, summary = wide_answer()
    r = results[1]
    volume = WIDE_SIZE[0] * WIDE_SIZE[1] * WIDE_SIZE[2]
    assert summary["jobs"] == 198000 and -(-volume // CHUNK) == 387 and summary["carved"] == 1 and r["voxels"] == volume - 1 and not after[1][1][-1, -1, -1]
    for value in (r["sum"][0], r["moment"][0], r["moment"][3], r["moment"][5]):
        assert int(value) > 1 << 32, "a model's sum past 2^32"
    x = WIDE_SIZE[0] - 1
    assert x * x > 1 << 32 and int(r["moment"][0]) == 6 * sum(v * v for v in range(WIDE_SIZE[0])) - x * x, "a single voxel's x^2 past 2^32; the sum by hand"
    assert 64 * (x - 63) > 1 << 22 and r["max"].tolist() == [WIDE_SIZE[0], 2, 3] and results[0]["voxels"] == 8 and not hit["carved"][0]
    return dict(jobs=summary["jobs"], chunks=1 + 387, sums=[int(r["sum"][0]), int(r["moment"][0]), int(r["moment"][3]), int(r["moment"][5])])


# ---- D. +-2^30 ---------------------------------------------------------------------------------------------------------------------------------------

def placements(lo, hi):
    """[(name, delta)]: the moves that bring the extent [lo, hi) to end exactly at +2^30 on each axis, to begin exactly at -2^30 on each axis, and
    into the corner (-2^30, -2^30, -2^30)."""
    out = []
    for axis in range(3):
        delta = [0, 0, 0]
        delta[axis] = LIMIT - int(hi[axis])
        out.append((f"ends at +2^30 on axis {axis}", delta))
    for axis in range(3):
        delta = [0, 0, 0]
        delta[axis] = -LIMIT - int(lo[axis])
        out.append((f"begins at -2^30 on axis {axis}", delta))
    out.append(("the corner at -2^30", [-LIMIT - int(lo[a]) for a in range(3)]))
    return out


def _fits(instances, delta):
    """Per instance: whether limitmodels.moved keeps its toModel.t within 2^46."""
    return [all(abs(int(t)) <= MAX_T for t in inst.toModel.t) for inst in L.moved(instances, delta)]


# D1. pair sweep

LIMIT_PAIR_CASES = ("thin shell", "-x", "+x", "-y", "+y", "-z", "+z", *pairsweepcases.TIES, "maps")


@functools.lru_cache(maxsize=None)
def limit_pair_sweeps():
    """[(name, the call at the origin, the call at the limit, the move, the pairs of the origin's call that were left out)]: the path cases of
    tests/pairsweepcases.py moved so that the boxes, a's after its motion among them, end exactly at +2^30 or begin exactly at -2^30.  A pair
    with an instance whose toModel.t the move would push past 2^46 is left out of both calls: with m = 2 a move of 2^30 is a t of 2^47, and
    in the corner the three moves add up for every map that turns, so of "maps" nothing is left there and the case is not made."""
    cases = []
    for name in LIMIT_PAIR_CASES:
        models, instances, pairs, motions = pairsweepcases.case(name)
        pairs, motions = np.asarray(pairs, dtype=np.int32).reshape(-1, 2), np.asarray(motions, dtype=np.int32).reshape(-1, 3)
        lo, hi = boxes_of(instances)
        ends = np.concatenate([lo, hi, lo[pairs[:, 0]] + motions, hi[pairs[:, 0]] + motions])
        for where, delta in placements(ends.min(axis=0), ends.max(axis=0)):
            fits = np.array(_fits(instances, delta))
            keep = fits[pairs[:, 0]] & fits[pairs[:, 1]]
            used = sorted(set(pairs[keep].ravel().tolist()))
            renamed = {k: n for n, k in enumerate(used)}
            kept_pairs = np.int32([[renamed[int(a)], renamed[int(b)]] for a, b in pairs[keep]])
            kept = [instances[k] for k in used]
            if not keep.any():  # (the corner of "maps": a turned map's rows sum to more than 1, and three moves of 2^30 pass 2^46)
                continue
            cases.append((f"{name}: {where}", (models, kept, kept_pairs, motions[keep]), (models, L.moved(kept, delta), kept_pairs, motions[keep]), delta,
                          np.nonzero(~keep)[0].tolist()))
    return cases


def shifted_pair_sweep(answer, delta):
    """A pair sweep's answer at the origin -> the answer after a move by `delta`: the sweeps are offsets and stay, the contacts are
    limitmodels.shifted_answer's."""
    sweeps, contacts, summary = answer
    shifted, _, _ = L.shifted_answer((contacts, np.zeros(0, dtype=paircontactsmodel.POINT_DTYPE), {}), delta)
    return sweeps, shifted, dict(summary)


def pair_sweep_model(call):
    models, instances, pairs, motions = call
    return pairsweepmodel.sweep(models, as_dicts(instances), pairs, motions)


def assert_limit_pair_sweep(case):
    name, origin, at_limit, delta, left_out = case
    models, instances, pairs, motions = at_limit
    lo, hi = boxes_of(instances)
    ends = np.concatenate([lo, hi, lo[pairs[:, 0]] + motions, hi[pairs[:, 0]] + motions])
    assert ends.min() >= -LIMIT and ends.max() <= LIMIT, name
    if name.startswith("maps"):
        kinds = list(pairsweepcases.MAPS)
        assert "corner" not in name and [kinds[p // 2] for p in left_out] == ["scale 1/2", "scale 1/2"], (name, left_out)
        assert len(pairs) == 8, "yaw, tilt, scale 1.5 and the mirror remain, on either body"
    else:
        assert left_out == [] and len(pairs) == len(origin[2])
    if "corner" in name:
        assert ends.min(axis=0).tolist() == [-LIMIT] * 3
    else:
        axis = int(name[-1])
        assert (ends[:, axis].max() == LIMIT) if "ends" in name else (ends[:, axis].min() == -LIMIT), name


@functools.lru_cache(maxsize=None)
def long_minified():
    """(models, instances, pairs, motions): one voxel moves (4096, -5, 2) and meets, about pose 4090 of its path, a 32^3 model minified to a body
    of 2^3 (toModel's m is 16 in units of 1, 2^20 in its own).  The kernel takes body b back along the path: the rows of b's m times the
    path's offsets pass 2^31 there, which the moves to +-2^30 cannot reach -- with such a map a move of 2^30 is a t of 2^50."""
    size = (32, 32, 32)
    v = (4096, -5, 2)
    there = sweepmodel.path(v)[4090][0]
    models = [pairsweepcases._full(size), pairsweepcases._full(pairsweepcases.VOXEL)]
    waiting = gpu.model_instance(forward_about_centre(0.0625 * np.eye(3), size, tuple(c + 1.0 for c in there)), size, 0, FILL)
    return models, [waiting, identity_at((0, 0, 0), pairsweepcases.VOXEL, 1, FILL)], np.int32([(1, 0)]), np.int32([v])


def assert_long_minified(answer):
    models, instances, pairs, motions = long_minified()
    s = answer[0]["sweep"][0]
    m = max(abs(int(c)) for row in instances[0].toModel.m for c in row)
    assert m == 16 << 16 and max(int(instances[0].boxMax[c]) - int(instances[0].boxMin[c]) for c in range(3)) <= 4
    assert 4000 < s["hit"] <= 4095 and m * int(s["at"][0]) >= 1 << 31, "a row of m times the offset of the touching pose passes 2^31"


# D2. brush

LIMIT_BRUSH_CASES = tuple(f"shape {s}" for s in modelbrushcases.SHAPES) + tuple(f"map {m}" for m in modelbrushcases.MAPS) + ("negative",)


def _stroke_points(stroke):
    """The points of a stroke that move with it: a and b of a box and a capsule, the centre a of a sphere and an ellipsoid."""
    return [list(stroke["a"])] + ([list(stroke["b"])] if stroke["shape"] in (gpu.SHAPE_BOX, gpu.SHAPE_CAPSULE) else [])


def moved_stroke(stroke, delta):
    out = dict(stroke, a=[int(stroke["a"][i]) + int(delta[i]) for i in range(3)])
    if stroke["shape"] in (gpu.SHAPE_BOX, gpu.SHAPE_CAPSULE):
        out["b"] = [int(stroke["b"][i]) + int(delta[i]) for i in range(3)]
    return out


@functools.lru_cache(maxsize=None)
def limit_brushes():
    """[(name, the call at the origin, the call at the limit, the move)]: the shape and map cases of tests/modelbrushcases.py moved, strokes and
    all, so that the extent of the boxes and of the strokes' centres and ends -- whichever reaches furthest -- ends exactly at +2^30 or begins
    exactly at -2^30; each with one more CARVE, a sphere of radius 3 whose centre lies on that end of the extent: exactly on +-2^30 after the
    move.  A case whose toModel.t the move would push past 2^46 is left out of that placement (the caller asserts which)."""
    cases = []
    for name in LIMIT_BRUSH_CASES:
        models, instances, strokes = modelbrushcases.case(name)
        lo, hi = boxes_of(instances)
        points = np.array([p for s in strokes for p in _stroke_points(s)], dtype=np.int64)
        low, high = np.minimum(lo.min(axis=0), points.min(axis=0)), np.maximum(hi.max(axis=0), points.max(axis=0))
        for where, delta in placements(low, high):
            if not all(_fits(instances, delta)):
                continue
            centre = [int(lo[0][a] + hi[0][a]) // 2 for a in range(3)]  # one more stroke: a sphere whose centre the move puts exactly on the limit
            for a in (range(3) if "corner" in where else [int(where[-1])]):
                centre[a] = int(high[a]) if "ends" in where else int(low[a])
            with_it = list(strokes) + [sphere(CARVE, centre, 3)]
            cases.append((f"{name}: {where}", (models, instances, with_it), (models, L.moved(instances, delta), [moved_stroke(s, delta) for s in with_it]), delta))
    return cases


def assert_limit_brushes(cases):
    names = [c[0] for c in cases]
    left_out = sorted({f"{n}: {w}" for n in LIMIT_BRUSH_CASES for w, _ in placements([0] * 3, [0] * 3)} - set(names))
    on_an_axis = [n for n in left_out if "corner" not in n]
    assert len(on_an_axis) == 6 and all(n.startswith("map minified 1/2") for n in on_an_axis), "along one axis only m = 2 passes 2^46"
    in_the_corner = sorted(n.split(":")[0] for n in names if "corner" in n)
    assert in_the_corner == ["map magnified 2", "map rotated 90", "map translated"], "in the corner the three moves add up for every map whose rows sum to more than 1"
    centre_on, box_on = 0, 0
    for name, origin, (models, instances, strokes), delta in cases:
        lo, hi = boxes_of(instances)
        centres = np.array([s["a"] for s in strokes if s["shape"] != gpu.SHAPE_BOX] or [[0, 0, 0]], dtype=np.int64)
        points = np.array([p for s in strokes for p in _stroke_points(s)], dtype=np.int64)
        assert lo.min() >= -LIMIT and hi.max() <= LIMIT and np.abs(points).max() <= LIMIT, name
        centre_on += int((np.abs(centres) == LIMIT).any())
        box_on += int((hi == LIMIT).any() or (lo == -LIMIT).any())
    assert centre_on == len(cases) and box_on >= 10, "a stroke centre exactly on +-2^30 in every call, and boxes that end or begin there"
    return left_out


# D3. world sweep

LIMIT_SWEEP_CASES = ("below the world", "sideways", "sideways open")
NEAR = 40  # "just outside" the 32^3 world: the near copy of a case lies this far from the world's origin


@functools.lru_cache(maxsize=None)
def limit_world_sweeps():
    """[(name, the call at the limit, the same call just outside the world, the move from the second to the first)]: the outside cases of
    tests/sweepcases.py moved along x and along z so that the boxes, after their motions too, end exactly at +2^30 or begin exactly at
    -2^30; and one voxel that moves 4096 along x and ends with its box at +2^30, coming down through y = 0 on the way.  Outside the world on x or z
    a column is its outside flags alone: the near copy, moved by a multiple of 64 from the far one, has the same answer but for the coordinates."""
    cases = []
    calls = [(name, sweepcases.case(name)) for name in LIMIT_SWEEP_CASES]
    calls.append(("4096 along x", ("thin", [sweepcases._full(sweepcases.VOXEL)], [identity_at((0, 4, 9), sweepcases.VOXEL, 0, 0)], [(4096, -6, 0)], DEFAULT)))
    for name, (key, models, instances, motions, so) in calls:
        lo, hi = boxes_of(instances)
        v = np.asarray(motions, dtype=np.int64)
        ends = np.concatenate([lo, hi, lo + v, hi + v])
        for axis in (0, 2):
            for sign in ((1, -1) if name != "4096 along x" else (1,)):
                if name == "4096 along x" and axis == 2:
                    continue
                far, near = [0, 0, 0], [0, 0, 0]
                far[axis] = (LIMIT - int(ends[:, axis].max())) if sign > 0 else (-LIMIT - int(ends[:, axis].min()))
                near[axis] = (NEAR - int(ends[:, axis].min())) if sign > 0 else (-NEAR - int(ends[:, axis].max()))
                where = f"{'ends at +2^30' if sign > 0 else 'begins at -2^30'} on axis {axis}"
                cases.append((f"{name}: {where}", (key, models, L.moved(instances, far), motions, so), (key, models, L.moved(instances, near), motions, so),
                              [far[a] - near[a] for a in range(3)]))
    return cases


def shifted_world_sweep(answer, delta):
    """A world sweep's answer -> the answer after a move by `delta` that changes no column the bodies meet: origin, min, max (where there is an
    overlap) and the points' voxels shifted."""
    sweeps, contacts, points, summary = answer
    contacts, points = contacts.copy(), points.copy()
    d = np.int32(delta)
    contacts["origin"] += d
    met = contacts["overlap"] > 0
    contacts["min"][met] += d
    contacts["max"][met] += d
    points["voxel"] += d
    return sweeps, contacts, points, dict(summary)


def assert_limit_world_sweep(case, want):
    name, (key, models, instances, motions, so), near, delta = case
    dims, solid, _ = sweepcases.world(key)
    lo, hi = boxes_of(instances)
    v = np.asarray(motions, dtype=np.int64)
    ends = np.concatenate([lo, hi, lo + v, hi + v])
    axis = int(name[-1])
    assert (ends[:, axis].max() == LIMIT) if "ends" in name else (ends[:, axis].min() == -LIMIT), name
    assert (ends[:, axis].min() >= dims[axis]) or (ends[:, axis].max() <= 0), "outside the world all the way"
    near_lo, near_hi = boxes_of(near[2])
    assert np.abs(np.concatenate([near_lo, near_hi, near_lo + v, near_hi + v])[:, axis]).min() >= dims[axis] and np.abs(near_lo).max() < 5000
    if name.startswith("4096"):
        s = want[0][0]
        assert s["steps"] == 4102 and s["hit"] > 3000 and s["axis"] == 1 and station_of(motions[0], int(s["hit"])) > 3000 and want[3]["jobs"] == 4097, s


# ---- F. the flight loop: carve, lift, brush in place, sweep, test, pick, draw, place -----------------------------------------------------------------

BRUSHED_POSES = ("slab tilted in the air", "ball high up", "pyramid in the air")  # one pose of every piece: the brush reaches every model
FLIGHT_PAINT = 0xFF00C0FF


def flight_brush(order):
    """(the three instances the brush goes through, the strokes in world coordinates): a capsule through the tilted slab, a PAINT on the side of the ball that faces
    flight_view and a CARVE below it, a box off a corner of the pyramid."""
    names = [p[0] for p in L.FLIGHT_POSES]
    instances = L.flight_instances(order)
    chosen = [instances[names.index(name)] for name in BRUSHED_POSES]
    (sx, sy, sz), (bx, by, bz), (px, py, pz) = [[int(c) for c in i.boxMin] for i in chosen]
    middle = [(int(chosen[0].boxMin[a]) + int(chosen[0].boxMax[a])) // 2 for a in range(3)]
    strokes = [capsule(CARVE, (middle[0] - 7, middle[1], middle[2]), (middle[0] + 7, middle[1] + 1, middle[2]), 1),
               sphere(PAINT, (bx + 5, by + 5, bz + 1), 3, FLIGHT_PAINT), sphere(CARVE, (bx + 5, by + 1, bz + 5), 2), box(CARVE, (px, py, pz), (px + 4, py + 3, pz + 5))]
    return chosen, strokes


def flight_velocities(instances):
    """Per pose an integer velocity towards the middle of them all (tests/test_gpu_model_sweep.py's flight loop), and the motion of the world
    sweep: the same, and 25 down."""
    centres = np.array([[(i.boxMin[c] + i.boxMax[c]) / 2 for c in range(3)] for i in instances])
    velocity = np.rint((centres.mean(axis=0) - centres) * 0.8).astype(np.int64)
    return velocity, velocity + np.int64([0, -25, 0])


def flight_pairs(instances):
    """(the pairs of the pair sweep, their motions): gpu.box_pairs with the largest velocity component as the margin, in both orders; v_a - v_b."""
    velocity, _ = flight_velocities(instances)
    pairs = gpu.box_pairs(instances, margin=int(np.abs(velocity).max()))
    pairs = np.concatenate([pairs, pairs[:, ::-1]])
    return pairs, velocity[pairs[:, 0]] - velocity[pairs[:, 1]]


def flight_view():
    """A view of the whole 64^3 world from in front of it (-z), a little off every symmetry."""
    from test_model_draw_cpu import looking_along_z
    return looking_along_z((30.3, 34.7, -58.2), 64, 64, 0.46, 0.46, skew=(0.02, -0.01))


def flight_references(models, order, pick_rules, draw_rules, tmp_path):
    """What the five read-only calls must give for the bodies `models` (in the device's order) over the world after the lift: world sweep, pair
    sweep and pair contacts from the numpy models, pick and draw from the host rules programs."""
    from test_model_contacts_cpu import model_of
    from test_model_draw_cpu import WORLD
    from test_model_draw_cpu import run_cases as run_draw
    from test_model_pick_cpu import run_cases as run_pick
    solid, colour = L.flight_after_lift()
    instances = L.flight_instances(order)
    dicts = as_dicts(instances)
    _, falling = flight_velocities(instances)
    sweeps = sweepmodel.sweep(solid, colour, models, dicts, falling, L.SOLID_OUTSIDE)
    sweeps[3]["jobs"] = sweepmodel.jobs(dicts, falling)
    pairs, motions = flight_pairs(instances)
    pair_sweeps = pairsweepmodel.sweep(models, dicts, pairs, motions)
    contacts = model_of(models, instances, gpu.box_pairs(instances))
    sub = tmp_path / f"references_{len(list(tmp_path.iterdir()))}"
    sub.mkdir()
    hits, _ = run_pick(pick_rules, sub, [(models, instances, L.flight_rays())])[0]
    frame = run_draw(draw_rules, sub, [dict(models=models, instances=instances, view=flight_view(), flags=WORLD, world=(solid, colour))])[0]
    return sweeps, pair_sweeps, contacts, hits, frame


def assert_the_brush_is_seen(before, after):
    """flight_references of the unbrushed and of the brushed bodies: at least one sweep, one pair and one pixel change."""
    assert (before[0][0]["hit"] != after[0][0]["hit"]).any() or before[0][1].tobytes() != after[0][1].tobytes(), "a world sweep or its contacts change"
    assert (before[1][0]["sweep"]["hit"] != after[1][0]["sweep"]["hit"]).any(), "a pair sweep changes"
    assert (before[2][0]["overlap"] != after[2][0]["overlap"]).any(), "a pair's overlap changes"
    assert (before[4][0] != after[4][0]).any() and (after[4][0] == FLIGHT_PAINT).any() and not (before[4][0] == FLIGHT_PAINT).any(), "a pixel shows the PAINT"
    assert (before[3]["argb"] != after[3]["argb"]).any() or (before[3]["t"].view(np.uint32) != after[3]["t"].view(np.uint32)).any(), "a pick changes"
