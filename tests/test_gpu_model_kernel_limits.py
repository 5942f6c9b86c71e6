"""GPU: cvxp_model_contacts and cvxq_model_pick at their kernels' compiled limits (the calls of tests/limitmodels.py; tests/test_limit_models_cpu.py
runs the same calls through the host rules programs and the numpy models).

Pair contacts are compared byte for byte with tests/paircontactsmodel.py (everything is integers).  Picks are compared byte for byte, on every
ray and through both entry points, with the host build of the rules (tests/model_pick_rules.cpp), and on the rays it calls unambiguous with
tests/modelpickmodel.py.  Every case asserts the property it is named after before it calls the device."""
import numpy as np
import pytest

import limitmodels as L
import modelpickmodel
import ruleslib
from cpuvox_amd import gpu
from test_gpu_model_contacts import _device_call as pair_device_call
from test_gpu_model_pick import _check as pick_check
from test_gpu_model_pick import _device_call as pick_device_call
from test_gpu_model_pick import _host_call as pick_host_call
from test_model_contacts_cpu import FILL, model_of, same, scene_cubes, scene_mixed
from test_model_pick_cpu import rays_of, run_cases
from test_world_contacts_cpu import CUBE, cube_model
from test_world_models_cpu import as_dicts, identity_at

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("model_limits_gpu"))


def _three_forms(ctx, scene, want, what):
    """The host form, the device form with the exact capacity and the device form with no list, against `want`."""
    models, instances, pairs = scene
    results, points, totals, ms = ctx.model_contacts(models, instances, pairs)
    assert ms > 0.0
    same((results, points, totals), want, what)
    same(pair_device_call(ctx, models, instances, pairs, want[2]["points"]), want, what + " (device)")
    got_results, listed, got_totals = pair_device_call(ctx, models, instances, pairs, 0)
    assert len(listed) == 0 and got_totals == want[2] and got_results.tobytes() == want[0].tobytes(), what + " (device, no list)"


# ---- A1. pair counts at the finish kernel's threads and the pair search's rounds ----------------------------------------------------------------------

@pytest.mark.parametrize("count", L.PAIR_COUNTS)
def test_pair_counts_at_the_finish_and_search_limits(ctx, count):
    """64 | 65 pairs: one and two of the finish kernel's threads; 4096 | 4097: two and three rounds of the pair search, 64 and 65 threads; 65536:
    every thread, with three runs of empty pairs longer than the first round's probe step."""
    call = L.cycled_answer(count)
    L.assert_cycled(count, call)
    models, instances, pairs, _, want = call
    _three_forms(ctx, (models, instances, pairs), want, f"{count} pairs")


# ---- A2. the random calls --------------------------------------------------------------------------------------------------------------------------

def test_the_random_calls_equal_the_model(ctx):
    calls = L.random_pair_calls()
    assert len(calls) == 160
    negative = sum(int((want[0]["pushA"] < 0).any() or (want[0]["pushB"] < 0).any()) for _, want in calls)
    without = sum(int(((want[0]["overlap"] > 0) & (want[0]["points"] == 0)).any() or (want[0]["overlap"] == 0).any()) for _, want in calls)
    assert negative > 40 and without > 20, "negative pushes (two's-complement adds) and words that stay zero (skipped adds)"
    for n, ((models, instances, pairs), want) in enumerate(calls):
        results, points, totals, _ = ctx.model_contacts(models, instances, pairs)
        same((results, points, totals), want, f"random call {n}")
        if n % 4 == 0:
            same(pair_device_call(ctx, models, instances, pairs, want[2]["points"]), want, f"random call {n} (device)")


# ---- A3. boxes at +-2^30 ---------------------------------------------------------------------------------------------------------------------------

def test_pair_boxes_at_the_coordinate_limit(ctx):
    for name, origin, at_limit, delta in L.limit_pair_cases():
        L.assert_limit_pair(name, at_limit, delta)
        want = model_of(*at_limit)
        assert want[0]["overlap"][0] > 0 and want[2]["points"] > 0, name
        same(want, L.shifted_answer(model_of(*origin), delta), name + ": the answer at the origin, shifted")
        _three_forms(ctx, at_limit, want, name)


# ---- A4. a small call after a large one ------------------------------------------------------------------------------------------------------------

def _with_capacity_4(context, scene):
    """The host and the device form with a list of four entries -> their bytes."""
    models, instances, pairs = scene
    results, points, totals, _ = context.model_contacts(models, instances, pairs, capacity=4)
    device_results, listed, device_totals = pair_device_call(context, models, instances, pairs, 4, spare=2)
    assert (listed[4:].view(np.uint8) == SENTINEL).all(), "nothing is written beyond the capacity"
    return results.tobytes(), points.tobytes(), totals, device_results.tobytes(), listed[:4].tobytes(), device_totals


def test_small_pair_calls_after_the_largest(ctx):
    """The 65536 call, then the two cubes, then the mixed call on one context, each with a list of four entries: the scratch a call gets may be
    what the larger call before it left."""
    models, instances, pairs, _, large = L.cycled_answer(65536)
    scenes = [(models, instances, pairs), scene_cubes(), scene_mixed()]
    wants = [large, model_of(*scenes[1]), model_of(*scenes[2])]
    assert len(scenes[1][2]) == 2 and len(scenes[2][2]) < 100 and all(w[2]["points"] > 4 for w in wants)
    fresh = []
    for scene in scenes:
        alone = gpu.Context(0)
        try:
            fresh.append(_with_capacity_4(alone, scene))
        finally:
            alone.close()
    for scene, want, alone in zip(scenes, wants, fresh):
        got = _with_capacity_4(ctx, scene)
        assert got == alone, "the bytes of a fresh context"
        assert got[0] == got[3] == want[0].tobytes() and got[1] == got[4] == want[1][:4].tobytes() and got[2] == got[5] == want[2]


# ---- B1. bodies deeper than 64 layers --------------------------------------------------------------------------------------------------------------

def test_long_bodies(ctx, rules, tmp_path):
    cases = [L.long_bodies(axis) for axis in range(3)]
    L.assert_long_bodies(cases, [hits for hits, _ in run_cases(rules, tmp_path, [case[:3] for case in cases])])
    for axis, (models, instances, rays, random) in enumerate(cases):
        got, _ = pick_check(ctx, rules, tmp_path, (models, instances, rays), f"long bodies along axis {axis}")
        subset = L.long_subset(axis)
        picked = rays[subset]
        model = modelpickmodel.pick_many(models, as_dicts(instances), picked["origin"], picked["direction"], picked["maxT"])
        share = modelpickmodel.compare(got[subset], model, f"long bodies along axis {axis}")
        print(f"long bodies along axis {axis}: the model calls {share:.4f} of the {len(subset)} rays unambiguous")
        assert share >= 0.95


# ---- B2. many jobs on one ray ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reverse", [False, True])
def test_the_crowded_row(ctx, rules, tmp_path, reverse):
    """64 boxes on every ray, duplicates, copies a voxel apart: jobs of one ray that end close together or tie exactly, whatever order the
    waves run in.  The reversed list is checked against the rules program's answer for the reversed list."""
    case = L.crowded_row(reverse)
    hits, jobs = run_cases(rules, tmp_path, [case])[0]
    n = [0]

    def run(cases):
        n[0] += 1
        sub = tmp_path / f"without_{n[0]}"
        sub.mkdir()
        return run_cases(rules, sub, cases)
    tied = L.row_ties(run, case, hits)
    L.assert_crowded_row(case, hits, jobs, tied)
    first, _ = pick_check(ctx, rules, tmp_path, case, f"the crowded row (reverse {reverse})")
    wrong = np.nonzero(first["instance"] != hits["instance"])[0]
    assert len(wrong) == 0, f"rays {wrong.tolist()} (tied: {tied[wrong].tolist()})"
    second, _ = pick_check(ctx, rules, tmp_path, case, f"the crowded row again (reverse {reverse})")
    assert first.tobytes() == second.tobytes() == hits.tobytes()


# ---- B3. the most instances and two scan chunks ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("copies", [False, True])
def test_the_most_instances_and_two_scan_chunks(ctx, rules, tmp_path, copies):
    case = L.cube_grid(copies)
    hits, jobs = run_cases(rules, tmp_path, [case])[0]
    L.assert_cube_grid(case, hits, jobs, copies)
    got, got_jobs = pick_check(ctx, rules, tmp_path, case, f"4096 instances (copies {copies})")
    assert got.tobytes() == hits.tobytes() and got_jobs == jobs


# ---- B4. boxes at +-2^30 ---------------------------------------------------------------------------------------------------------------------------

def test_pick_boxes_at_the_coordinate_limit(ctx, rules, tmp_path):
    for n, case in enumerate(L.limit_pick_cases()):
        sub = tmp_path / f"case_{n}"
        sub.mkdir()
        got, _ = pick_check(ctx, rules, sub, case[1:4], case[0])
        L.assert_limit_pick(case, got)


# ---- B5. a small call after a large one ------------------------------------------------------------------------------------------------------------

def test_small_picks_after_the_largest(ctx, rules, tmp_path):
    """4096 instances and two scan chunks, then test_gpu_model_pick.py's cube by hand, then one ray against one instance, on one context."""
    cube = ([cube_model()], [identity_at((10, 10, 10), CUBE, 0, FILL)],
            rays_of([(5, 11.5, 12.5), (20, 11.5, 12.5), (11.5, 2, 12.5), (11.5, 30, 12.5), (11.5, 12.5, 0), (11.5, 12.5, 15.5)],
                    [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -2, 0), (0, 0, 1), (0, 0, -0.5)], 100))
    cases = [L.cube_grid(False), cube, (cube[0], cube[1], cube[2][3:4])]
    want = [hits for hits, _ in run_cases(rules, tmp_path, cases)]
    assert want[1]["t"].tolist() == [5.0, 6.0, 8.0, 8.0, 10.0, 3.0] and want[2]["voxel"].tolist() == [[11, 13, 12]] and (want[0]["instance"] >= 0).sum() > 30
    fresh = []
    for case in cases:
        alone = gpu.Context(0)
        try:
            fresh.append((pick_host_call(alone, *case).tobytes(), pick_device_call(alone, *case).tobytes()))
        finally:
            alone.close()
    for case, hits, alone in zip(cases, want, fresh):
        got = (pick_host_call(ctx, *case).tobytes(), pick_device_call(ctx, *case).tobytes())
        assert got == alone and got[0] == got[1] == hits.tobytes()
