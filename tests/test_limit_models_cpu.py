"""CPU (no GPU needed): the calls of tests/limitmodels.py have the properties they are named after, and the host rules programs
(tests/pair_contacts_rules.cpp, tests/model_pick_rules.cpp: the scalar rule AND the wave's walk, which must agree in every byte) equal the numpy
models on them.  tests/test_gpu_model_kernel_limits.py and tests/test_gpu_model_sequences.py run the same calls on the device; they repeat
the cheap assertions before they call it.  Every property comes from the numpy models, the rules programs or plain arithmetic."""
import numpy as np
import pytest

import contactsmodel
import limitmodels as L
import modelpickmodel
import modelsmodel
import pickmodel
import ruleslib
from cpuvox_amd import gpu
from test_model_contacts_cpu import model_of, same, scene_cubes
from test_model_contacts_cpu import run_cases as run_pair_cases
from test_model_pick_cpu import run_cases as run_pick_cases
from test_world_models_cpu import as_dicts


@pytest.fixture(scope="module")
def pair_rules(tmp_path_factory):
    return ruleslib.build("pair_contacts_rules", tmp_path_factory.mktemp("limit_pairs"))


@pytest.fixture(scope="module")
def pick_rules(tmp_path_factory):
    return ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("limit_pick"))


# ---- A. cvxp_model_contacts -------------------------------------------------------------------------------------------------------------------------

def test_the_lattice_has_pairs_of_every_kind_and_no_two_alike():
    L.assert_lattice_base()


def test_the_tiling_helper_equals_the_model(pair_rules, tmp_path):
    """On a call of 2 D + 5 cycled pairs with a run of empty pairs inside: the helper's answer is model_of's, and the rules program's."""
    _, _, base, d, base_answer = L.lattice_base()
    count = 2 * d + 5
    runs = [(d + 3, d + 40)]
    models, instances, pairs, which = L.cycled_call(count, runs)
    assert len(pairs) == count >= 2 * d + 5 and (which[runs[0][0]:runs[0][1]] >= d).all() and (which[:runs[0][0]] < d).all() and (which[runs[0][1]:] < d).all()
    tiled = L.tile_answer(base_answer, L.pair_jobs(instances, base), which)
    same(tiled, model_of(models, instances, pairs), "the tiling helper")
    assert not tiled[0]["overlap"][runs[0][0]:runs[0][1]].any() and tiled[0]["firstPoint"][runs[0][1]] == tiled[0]["firstPoint"][runs[0][0]] > 0
    same(run_pair_cases(pair_rules, tmp_path, [(models, instances, pairs)])[0], tiled, "the rules program")


@pytest.mark.parametrize("count", L.PAIR_COUNTS)
def test_pair_counts_at_the_finish_and_search_limits(pair_rules, tmp_path, count):
    call = L.cycled_answer(count)
    L.assert_cycled(count, call)
    models, instances, pairs, _, want = call
    same(run_pair_cases(pair_rules, tmp_path, [(models, instances, pairs)])[0], want, f"{count} pairs")


def test_pair_boxes_at_the_coordinate_limit(pair_rules, tmp_path):
    cases = L.limit_pair_cases()
    assert len(cases) == 9
    got = run_pair_cases(pair_rules, tmp_path, [at_limit for _, _, at_limit, _ in cases])
    for (name, origin, at_limit, delta), g in zip(cases, got):
        L.assert_limit_pair(name, at_limit, delta)
        want = model_of(*at_limit)
        assert want[0]["overlap"][0] > 0 and want[2]["points"] > 0, name
        same(want, L.shifted_answer(model_of(*origin), delta), name + ": the answer at the origin, shifted")
        same(g, want, name)
    assert model_of(*cases[0][1])[0].tobytes() == model_of(*scene_cubes())[0].tobytes()


# ---- B. cvxq_model_pick -----------------------------------------------------------------------------------------------------------------------------

def test_long_bodies_are_hit_deep_and_the_rules_equal_the_model(pick_rules, tmp_path):
    cases = [L.long_bodies(axis) for axis in range(3)]
    got = run_pick_cases(pick_rules, tmp_path, [case[:3] for case in cases])
    L.assert_long_bodies(cases, [hits for hits, _ in got])
    for axis, (case, (hits, jobs)) in enumerate(zip(cases, got)):
        models, instances, rays, random = case
        subset = L.long_subset(axis)
        assert len(subset) == L.LONG_SUBSET and random[subset].all() and jobs > len(rays)
        picked = rays[subset]
        model = modelpickmodel.pick_many(models, as_dicts(instances), picked["origin"], picked["direction"], picked["maxT"])
        assert (~model[1]).mean() >= 0.95, f"axis {axis}: the model calls {(~model[1]).mean():.3f} of the subset unambiguous"
        assert modelpickmodel.compare(hits[subset], model, f"long bodies along axis {axis}") >= 0.95


@pytest.mark.parametrize("reverse", [False, True])
def test_the_crowded_row_has_many_jobs_many_winners_and_ties(pick_rules, tmp_path, reverse):
    case = L.crowded_row(reverse)
    hits, jobs = run_pick_cases(pick_rules, tmp_path, [case])[0]
    n = [0]

    def run(cases):
        n[0] += 1
        sub = tmp_path / f"without_{n[0]}"
        sub.mkdir()
        return run_pick_cases(pick_rules, sub, cases)
    L.assert_crowded_row(case, hits, jobs, L.row_ties(run, case, hits))
    if reverse:
        forward, _ = run_pick_cases(pick_rules, tmp_path, [L.crowded_row(False)])[0]
        assert hits["t"].tobytes() == forward["t"].tobytes(), "the reversed list changes no ray's t (a tie may go to another instance's voxel)"
        assert (hits["instance"][hits["instance"] >= 0] != 63 - forward["instance"][forward["instance"] >= 0]).any(), "but renaming the indices is not the answer: ties go to the lower index"


@pytest.mark.parametrize("copies", [False, True])
def test_the_most_instances_and_two_scan_chunks(pick_rules, tmp_path, copies):
    case = L.cube_grid(copies)
    hits, jobs = run_pick_cases(pick_rules, tmp_path, [case])[0]
    L.assert_cube_grid(case, hits, jobs, copies)


def test_pick_boxes_at_the_coordinate_limit(pick_rules, tmp_path):
    cases = L.limit_pick_cases()
    assert len(cases) == 7
    got = run_pick_cases(pick_rules, tmp_path, [case[1:4] for case in cases])
    for case, (hits, _) in zip(cases, got):
        L.assert_limit_pick(case, hits)
        rays = case[3]
        assert (rays["origin"].astype(np.float64) % 0.5 == 0).all(), "the origins are exact"


# ---- C. the flight loop -----------------------------------------------------------------------------------------------------------------------------

ORDER = ("slab", "pyramid", "ball")


def _flight():
    pieces = L.flight_world()[3]
    models = [(pieces[name][2], pieces[name][3]) for name in ORDER]
    instances = L.flight_instances(ORDER)
    return pieces, models, instances, gpu.box_pairs(instances)


def test_the_flight_world_has_three_heads_and_an_odd_offset():
    solid, colour, neck, pieces = L.flight_world()
    volumes = {name: p[1][0] * p[1][1] * p[1][2] for name, p in pieces.items()}
    assert sum(v % 2 for v in volumes.values()) == 2, "two odd volumes: in whatever order the pieces are stored, one that is not the first starts at an odd byte"
    assert any(v % 4 for v in volumes.values()) and len({p[3].sum() for p in pieces.values()}) == 3 and len({tuple(p[1]) for p in pieces.values()}) == 3
    after, after_colour = L.flight_after_lift()
    assert not after[:, L.NECK[0]:, :].any() and after[:, :L.GROUND, :].all() and after[:, L.GROUND:L.NECK[0], :].sum() == 3 * 16 * (L.NECK[0] - L.GROUND)
    for name, (lo, size, argb, mask) in pieces.items():
        box = tuple(slice(lo[a], lo[a] + size[a]) for a in range(3))
        assert lo[1] == L.NECK[1] and (solid[box].transpose(0, 2, 1) >= mask).all() and (argb[mask] == colour[box].transpose(0, 2, 1)[mask]).all() and not argb[~mask].any()


def test_the_flight_poses_rest_overlap_touch_and_fly(pair_rules, pick_rules, tmp_path):
    pieces, models, instances, pairs = _flight()
    solid, colour = L.flight_after_lift()
    want_world = contactsmodel.contacts(solid, colour, models, as_dicts(instances), L.SOLID_OUTSIDE)
    want_pairs = model_of(models, instances, pairs)
    free = L.assert_flight_poses(want_world, want_pairs, pairs)
    assert len(instances) == len(L.FLIGHT_POSES) >= 12 and len(free) >= 3
    same(run_pair_cases(pair_rules, tmp_path, [(models, instances, pairs)])[0], want_pairs, "the poses' pairs")
    rays = L.flight_rays()
    hits, jobs = run_pick_cases(pick_rules, tmp_path, [(models, instances, rays)])[0]
    assert jobs > len(rays) and (hits["instance"] >= 0).sum() > 100 and len(set(hits["instance"].tolist())) > 8
    model = modelpickmodel.pick_many(models, as_dicts(instances), rays["origin"], rays["direction"], rays["maxT"])
    assert modelpickmodel.compare(hits, model, "the poses") >= 0.9


def test_a_pick_after_placing_is_the_nearer_of_world_and_bodies():
    """At the level of the models: pickmodel over the world with the free poses filled in equals, ray by ray, the nearer of pickmodel over the world
    before and modelpickmodel over the placed poses, on the rays both call unambiguous, and those are at least 90 %."""
    pieces, models, instances, pairs = _flight()
    solid, colour = L.flight_after_lift()
    free = L.assert_flight_poses(contactsmodel.contacts(solid, colour, models, as_dicts(instances), L.SOLID_OUTSIDE), model_of(models, instances, pairs), pairs)
    placed = as_dicts([instances[k] for k in free])
    rays = L.flight_rays()
    o, d, max_t = rays["origin"], rays["direction"], rays["maxT"]
    world = pickmodel.pick_many(solid, colour, o, d, max_t)
    bodies, amb = modelpickmodel.pick_many(models, placed, o, d, max_t)
    both = (world[1] >= 0) & (bodies["instance"] >= 0)
    close = both & (np.abs(world[3] - bodies["t"]) * np.linalg.norm(d.astype(np.float64), axis=1) < pickmodel.EPS)
    ok = ~(world[4] | amb | close)
    assert ok.mean() >= 0.9, f"{ok.mean():.4f} of the rays are unambiguous"
    from_bodies = (bodies["instance"] >= 0) & ((world[1] < 0) | (bodies["t"] < world[3]))
    assert (from_bodies & ok).sum() > 20 and (~from_bodies & (world[1] >= 0) & ok).sum() > 20, "both sources win somewhere"
    after = pickmodel.pick_many(*modelsmodel.place(solid, colour, models, placed), o, d, max_t)
    sure = ok & ~after[4]
    assert sure.mean() >= 0.85
    assert (after[0][sure] == np.where(from_bodies[:, None], bodies["voxel"], world[0])[sure]).all() and (after[1][sure] == np.where(from_bodies, bodies["face"], world[1])[sure]).all()
    assert (after[2][sure] == np.where(from_bodies, bodies["argb"], world[2])[sure]).all() and np.allclose(after[3][sure], np.where(from_bodies, bodies["t"], world[3])[sure], rtol=1e-9, atol=1e-9)
