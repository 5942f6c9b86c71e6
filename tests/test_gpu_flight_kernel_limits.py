"""GPU: cvxs_world_sweep, cvxm_pair_sweep and cvxd_models_brush at their kernels' compiled limits (the calls of tests/limitflight.py;
tests/test_limit_flight_cpu.py runs the same calls through the host rules programs and the numpy models): more jobs than a launch has waves,
every list word and list row, model volumes on and beside the chunk and step edges, sums past 2^32, coordinates at +-2^30, and a small call
after the largest on one context.

Every call goes through the host entry point and the _device entry point, and both are compared byte for byte with the numpy model
(tests/sweepmodel.py, tests/pairsweepmodel.py, tests/modelbrushmodel.py): everything is integers, so there is no tolerance.  Every case asserts
the property it is named after before it calls the device."""
import numpy as np
import pytest

import limitflight as F
import modelbrushcases
import pairsweepcases
import sweepcases
from cpuvox_amd import gpu
from test_gpu_model_brush import _back, _both
from test_gpu_model_sweep import _device_call as pair_device_call
from test_gpu_world_contacts import SENTINEL, World
from test_gpu_world_dense import _any_world
from test_gpu_world_sweep import _device_call as sweep_device_call
from test_model_sweep_cpu import same as same_pairs
from test_world_sweep_cpu import same as same_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(key):
        if key not in made:
            made[key] = World(*sweepcases.world(key))
        return made[key]
    yield get
    for w in made.values():
        w.close()


def _sweep_both(context, call, want, what):
    """cvxs_world_sweep and cvxs_world_sweep_device (into sentinel-filled tensors, the list with the exact capacity) against `want`."""
    _, models, instances, motions, so = call
    sweeps, contacts, points, totals, ms = context.world_sweep(models, instances, motions, so)
    assert ms > 0.0
    same_sweep((sweeps, contacts, points, totals), want, what)
    n = want[3]["points"]
    got = sweep_device_call(context, models, instances, motions, so, n)
    same_sweep((got[0], got[1], got[2][:n], got[3]), want, what + " (device)")
    assert (got[2][n:].view(np.uint8) == SENTINEL).all(), "entries beyond the capacity keep what they held"
    return (sweeps.tobytes(), contacts.tobytes(), points.tobytes(), totals, got[0].tobytes(), got[1].tobytes(), got[2][:n].tobytes(), got[3])


def _pairs_both(context, call, want, what):
    """cvxm_pair_sweep and cvxm_pair_sweep_device (into a sentinel-filled tensor; with and without contacts) against `want`."""
    models, instances, pairs, motions = call[:4]
    n = len(pairs)
    sweeps, contacts, totals, ms = context.model_sweep(models, instances, pairs, motions)
    assert ms > 0.0
    same_pairs((sweeps, contacts, totals), want, what)
    got = pair_device_call(context, models, instances, pairs, motions)
    same_pairs((got[0], got[1][:n], got[2]), want, what + " (device)")
    assert (got[1][n:].view(np.uint8) == SENTINEL).all(), "entries beyond the pairs keep what they held"
    return (sweeps.tobytes(), contacts.tobytes(), totals, got[0].tobytes(), got[1][:n].tobytes(), got[2])


def _brush_both(context, call, want, what):
    """cvxd_models_brush and cvxd_models_brush_device (test_gpu_model_brush._both) against `want` -> the bytes of both."""
    after, results, hit, totals, tensors = _both(context, call[0], call[1], call[2], want, what)
    arrays = b"".join((a.tobytes() if a is not None else b"") + (m.tobytes() if m is not None else b"") for a, m in list(after) + _back(tensors))
    return (arrays, results.tobytes(), hit.tobytes(), totals)


# ---- A. cvxs_world_sweep -----------------------------------------------------------------------------------------------------------------------------

def test_more_than_2_18_sweep_jobs_forwards_and_backwards(worlds):
    """276 480 (instance, column, station) jobs on 2^18 waves: the bodies at the end of the list are swept by waves on their second job, and
    one body's jobs straddle the turn.  Reversed, the same bodies come first."""
    F.assert_many_stations()
    forward, back = F.sweep_answer(), F.sweep_answer(True)
    F.assert_reversed_sweep(forward, back)
    context = worlds("terrain").ctx
    _sweep_both(context, F.many_stations(), forward, "72 bodies of 60 stations")
    _sweep_both(context, F.many_stations(True), back, "72 bodies of 60 stations, reversed")


def test_world_sweeps_at_the_coordinate_limit(worlds):
    for case in F.limit_world_sweeps():
        name, at_limit, near, delta = case
        want = F.world_sweep_model(*at_limit)
        F.assert_limit_world_sweep(case, want)
        same_sweep(F.shifted_world_sweep(F.world_sweep_model(*near), delta), want, name + ": the answer just outside the world, shifted")
        _sweep_both(worlds(at_limit[0]).ctx, at_limit, want, name)


# ---- B. cvxm_pair_sweep ------------------------------------------------------------------------------------------------------------------------------

def test_more_than_2_18_pair_jobs(ctx):
    """268 800 (pair, column) jobs: the last 100 pairs are swept by waves on their second job."""
    F.assert_pair_units()
    F.assert_many_pair_jobs()
    call = F.many_pair_jobs()
    _pairs_both(ctx, call, call[4], "4200 pairs of 64 jobs")


def test_runs_of_pairs_without_jobs(ctx):
    """65536 pairs with three runs of 1100 and more job-less ones: the search for a job's pair meets a flat prefix longer than its probe step."""
    F.assert_pair_units(F.SMALL_SIZE)
    F.assert_pair_empty_runs()
    call = F.pair_empty_runs()
    _pairs_both(ctx, call, call[4], "65536 pairs with three runs of job-less ones")


def test_pair_sweeps_at_the_coordinate_limit(ctx):
    cases = F.limit_pair_sweeps()
    assert len(cases) == 7 * len(F.LIMIT_PAIR_CASES) - 1
    origins = {}
    for case in cases:
        name, origin, at_limit, delta, _ = case
        F.assert_limit_pair_sweep(case)
        key = (name.split(":")[0], len(origin[2]))
        if key not in origins:
            origins[key] = F.pair_sweep_model(origin)
        want = F.shifted_pair_sweep(origins[key], delta)
        assert (want[0]["sweep"]["hit"] > 0).any(), name
        _pairs_both(ctx, at_limit, want, name)


def test_a_long_motion_under_a_minified_map(ctx):
    call = F.long_minified()
    want = F.pair_sweep_model(call)
    F.assert_long_minified(want)
    _pairs_both(ctx, call, want, "4096 along x under a map of 16")


# ---- C. cvxd_models_brush ----------------------------------------------------------------------------------------------------------------------------

def test_more_than_2_18_mark_jobs(ctx):
    """270 000 (instance, column) jobs: bodies 292 .. 299, each under a stroke of its own, are marked by waves on their second job."""
    F.assert_many_mark_jobs()
    _brush_both(ctx, F.many_mark_jobs(), F.mark_answer(), "300 bodies of 900 columns")


@pytest.mark.parametrize("bodies", F.ROW_BODIES)
@pytest.mark.parametrize("strokes", F.ROW_STROKES)
def test_list_rows(ctx, strokes, bodies):
    """Two, three and 64 list words an instance, and more than one instance: row k of the lists begins at word k * words."""
    F.assert_list_rows(strokes, bodies)
    _brush_both(ctx, F.list_rows(strokes, bodies), F.rows_answer(strokes, bodies), f"{strokes} strokes, {bodies} bodies")


def test_chunk_edges(ctx):
    """Eight models of 1 .. 3 chunks in one call: the chunk of a job is its index less the chunks of the models before; the last chunk ends
    on, one before and one behind a step of 64."""
    F.assert_chunk_edges()
    _brush_both(ctx, F.chunk_edges(), F.edges_answer(), "eight models at the chunk edges")


def test_wide_sums(ctx):
    """A coordinate product, a wave's sum and a model's sums past 2^32."""
    F.assert_wide_sums()
    _brush_both(ctx, F.wide_sums(), F.wide_answer(), "a model 66000 long")


def test_brushes_at_the_coordinate_limit(ctx):
    cases = F.limit_brushes()
    F.assert_limit_brushes(cases)
    for name, origin, at_limit, delta in cases:
        want = F.brush_model(*origin)
        assert want[3]["carved"] > 0, name
        _brush_both(ctx, at_limit, want, name)


# ---- E. a small call after a large one -----------------------------------------------------------------------------------------------------------------

def test_small_world_sweeps_after_the_largest():
    """The 276 480 jobs on the terrain, then the thin shell and one voxel below the world on the 32^3 world uploaded into the SAME context:
    first[] and the stations of a call may lie where the larger call before it left its own."""
    calls = [F.many_stations(), sweepcases.case("thin shell"), sweepcases.case("below the world")]
    wants = [F.sweep_answer(), sweepcases.answer("thin shell"), sweepcases.answer("below the world")]
    assert len(calls[1][2]) == 1 and len(calls[2][2]) == 1 and wants[0][3]["jobs"] > F.TURN > wants[1][3]["jobs"] == 64 > wants[2][3]["jobs"] == 1
    fresh = []
    for call, want in zip(calls, wants):
        alone = World(*sweepcases.world(call[0]))
        try:
            fresh.append(_sweep_both(alone.ctx, call, want, "a fresh context"))
        finally:
            alone.close()
    shared = World(*sweepcases.world("terrain"))
    thin = _any_world(*sweepcases.world("thin"))
    try:
        for n, (call, want, alone) in enumerate(zip(calls, wants, fresh)):
            if n == 1:
                shared.ctx.upload_world(thin)
            assert _sweep_both(shared.ctx, call, want, f"call {n} on one context") == alone, "the bytes of a fresh context"
    finally:
        shared.close()
        thin.close()


def test_small_pair_sweeps_after_the_largest(ctx):
    """65536 pairs and 248 544 jobs, then the thin shell, then one pair of voxels, on one context."""
    large = F.pair_empty_runs()
    calls = [large, pairsweepcases.case("thin shell"), pairsweepcases.case("1 pairs")]
    wants = [large[4], pairsweepcases.answer("thin shell"), pairsweepcases.answer("1 pairs")]
    assert len(calls[1][2]) == 1 and len(calls[2][2]) == 1 and wants[1][0]["sweep"]["hit"][0] == 4
    fresh = []
    for call, want in zip(calls, wants):
        alone = gpu.Context(0)
        try:
            fresh.append(_pairs_both(alone, call, want, "a fresh context"))
        finally:
            alone.close()
    for n, (call, want, alone) in enumerate(zip(calls, wants, fresh)):
        assert _pairs_both(ctx, call, want, f"call {n} on one context") == alone, "the bytes of a fresh context"


def test_small_brushes_after_the_largest(ctx):
    """270 000 mark jobs and 5400 elements of keys, then the model 66000 long (396 008 elements), then `same voxel`, then one voxel under one
    stroke, on one context: the key array a call gets may be what a larger call before it left."""
    calls = [F.many_mark_jobs(), F.wide_sums(), modelbrushcases.case("same voxel"), modelbrushcases.case("carve")]
    wants = [F.mark_answer(), F.wide_answer(), modelbrushcases.answer("same voxel"), modelbrushcases.answer("carve")]
    assert len(calls[3][1]) == 1 and len(calls[3][2]) == 1 and wants[3][1]["carved"][0] == 1 and wants[2][1]["painted"][0] == 1
    fresh = []
    for call, want in zip(calls, wants):
        alone = gpu.Context(0)
        try:
            fresh.append(_brush_both(alone, call, want, "a fresh context"))
        finally:
            alone.close()
    for n, (call, want, alone) in enumerate(zip(calls, wants, fresh)):
        assert _brush_both(ctx, call, want, f"call {n} on one context") == alone, "the bytes of a fresh context"
