"""CPU (no GPU needed): the calls of tests/limitflight.py have the properties they are named after, and the host rules programs
(tests/sweep_rules.cpp, tests/pair_sweep_rules.cpp, tests/model_brush_rules.cpp: the rule AND the kernels' walk with the lanes taken in turn,
which must agree in every byte) equal the numpy models on them.  tests/test_gpu_flight_kernel_limits.py and tests/test_gpu_flight_sequences.py
run the same calls on the device; they repeat the cheap assertions before they call it.  Every property comes from the numpy models,
sweepmodel.jobs / pairsweepmodel.pair_jobs or plain prefix arithmetic; everything is integers, so no comparison has a tolerance."""
import numpy as np
import pytest

import limitflight as F
import limitmodels as L
import modelbrushcases
import pairsweepcases
import pairsweepmodel
import ruleslib
import sweepcases
from test_model_brush_cpu import parse as parse_brush
from test_model_brush_cpu import same as same_brush
from test_model_brush_cpu import size_of
from test_model_brush_cpu import words_of as brush_words
from test_model_sweep_cpu import parse as parse_pairs
from test_model_sweep_cpu import same as same_pairs
from test_model_sweep_cpu import words_of as pair_words
from test_world_models_cpu import as_dicts
from test_world_sweep_cpu import run_world
from test_world_sweep_cpu import same as same_sweep


@pytest.fixture(scope="module")
def sweep_rules(tmp_path_factory):
    return ruleslib.build("sweep_rules", tmp_path_factory.mktemp("limit_sweep"))


@pytest.fixture(scope="module")
def pair_rules(tmp_path_factory):
    return ruleslib.build("pair_sweep_rules", tmp_path_factory.mktemp("limit_pair_sweep"))


@pytest.fixture(scope="module")
def brush_rules(tmp_path_factory):
    return ruleslib.build("model_brush_rules", tmp_path_factory.mktemp("limit_brush"))


def run_pairs(rules, tmp_path, calls):
    """Pair-sweep calls (models, instances, pairs, motions, ...) through the rules program in one run -> their (sweeps, contacts, summary)."""
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *[pair_words(*call[:4]) for call in calls], dtype=np.uint8).tobytes()
    out, at = [], 0
    for call in calls:
        size = 200 * len(call[2]) + 32
        out.append(parse_pairs(raw[at:at + size], len(call[2])))
        at += size
    assert at == len(raw)
    return out


def run_brushes(rules, tmp_path, calls):
    """Brush calls (models, instances, strokes, ...) through the rules program in one run -> their (models after, results, hits, summary)."""
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *[brush_words(*call[:3]) for call in calls], dtype=np.uint8).tobytes()
    out, at = [], 0
    for call in calls:
        size = size_of(call[0], call[1])
        out.append(parse_brush(raw[at:at + size], call[0], call[1]))
        at += size
    assert at == len(raw)
    return out


# ---- A. cvxs_world_sweep -----------------------------------------------------------------------------------------------------------------------------

def test_more_than_2_18_sweep_jobs_forwards_and_backwards(sweep_rules, tmp_path):
    counts = F.assert_many_stations()
    print(f"A1: {counts}")
    forward, back = F.sweep_answer(), F.sweep_answer(True)
    F.assert_reversed_sweep(forward, back)
    same_sweep(run_world(sweep_rules, tmp_path, *F.many_stations()), forward, "72 bodies of 60 stations")
    same_sweep(run_world(sweep_rules, tmp_path, *F.many_stations(True)), back, "72 bodies of 60 stations, reversed")


def test_world_sweeps_at_the_coordinate_limit(sweep_rules, tmp_path):
    cases = F.limit_world_sweeps()
    assert len(cases) == 13
    for n, case in enumerate(cases):
        name, at_limit, near, delta = case
        want = F.world_sweep_model(*at_limit)
        F.assert_limit_world_sweep(case, want)
        assert delta[1] == 0 and sum(1 for d in delta if d) == 1
        shifted = F.shifted_world_sweep(F.world_sweep_model(*near), delta)
        same_sweep(shifted, want, name + ": the answer just outside the world, shifted")
        sub = tmp_path / f"case_{n}"
        sub.mkdir()
        same_sweep(run_world(sweep_rules, sub, *at_limit), want, name)
    for name in F.LIMIT_SWEEP_CASES:  # the moved cases keep what the cases at home are named for
        home = sweepcases.answer(name)[0]
        for case in cases:
            if case[0].startswith(name + ":") and name != "sideways":
                assert F.world_sweep_model(*case[1])[0]["hit"].tolist() == home["hit"].tolist(), case[0]


# ---- B. cvxm_pair_sweep ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [F.PAIR_SIZE, F.SMALL_SIZE])
def test_the_pair_units_and_the_tiling_helper(pair_rules, tmp_path, size):
    """The units have the properties the large calls rely on, and on a call of 2 D + 9 units with a run of job-less ones inside the helper's
    answer is pairsweepmodel.sweep's, and the rules program's."""
    F.assert_pair_units(size)
    d = F.pair_units(size)[4]
    which = np.concatenate([np.arange(d), [d, d + 1, d, d + 1], np.arange(d)[::-1], np.arange(5)])
    call = F.tiled_pair_call(which, size)
    models, instances, pairs, motions, tiled = call
    same_pairs(tiled, pairsweepmodel.sweep(models, as_dicts(instances), pairs, motions), "the tiling helper")
    assert tiled[1]["firstPoint"][-1] > 0 and tiled[2]["jobs"] == (2 * d + 5) * size[0] * size[2]
    same_pairs(run_pairs(pair_rules, tmp_path, [call])[0], tiled, "the rules program")


def test_more_than_2_18_pair_jobs(pair_rules, tmp_path):
    print(f"B1: {F.assert_many_pair_jobs()}")
    call = F.many_pair_jobs()
    same_pairs(run_pairs(pair_rules, tmp_path, [call])[0], call[4], "4200 pairs of 64 jobs")


def test_runs_of_pairs_without_jobs(pair_rules, tmp_path):
    print(f"B2: {F.assert_pair_empty_runs()}")
    call = F.pair_empty_runs()
    same_pairs(run_pairs(pair_rules, tmp_path, [call])[0], call[4], "65536 pairs with three runs of job-less ones")


def test_pair_sweeps_at_the_coordinate_limit(pair_rules, tmp_path):
    cases = F.limit_pair_sweeps()
    assert len(cases) == 7 * len(F.LIMIT_PAIR_CASES) - 1, "every placement of every case but the corner of `maps`"
    got = run_pairs(pair_rules, tmp_path, [at_limit for _, _, at_limit, _, _ in cases])
    for case, g in zip(cases, got):
        name, origin, at_limit, delta, _ = case
        F.assert_limit_pair_sweep(case)
        want = F.shifted_pair_sweep(F.pair_sweep_model(origin), delta)
        same_pairs(F.pair_sweep_model(at_limit), want, name + ": the answer at the origin, shifted")
        assert (want[0]["sweep"]["hit"] > 0).any(), name
        same_pairs(g, want, name)
    for name in F.LIMIT_PAIR_CASES[:-1]:  # where no pair is left out the sweeps are the case's own
        home = pairsweepcases.answer(name)[0]
        assert all(F.pair_sweep_model(c[1])[0].tobytes() == home.tobytes() for c in cases if c[0].startswith(name + ":"))


def test_a_long_motion_under_a_minified_map(pair_rules, tmp_path):
    call = F.long_minified()
    want = F.pair_sweep_model(call)
    F.assert_long_minified(want)
    same_pairs(run_pairs(pair_rules, tmp_path, [call])[0], want, "4096 along x under a map of 16")


# ---- C. cvxd_models_brush ----------------------------------------------------------------------------------------------------------------------------

def test_more_than_2_18_mark_jobs(brush_rules, tmp_path):
    print(f"C1: {F.assert_many_mark_jobs()}")
    same_brush(run_brushes(brush_rules, tmp_path, [F.many_mark_jobs()])[0], F.mark_answer(), "300 bodies of 900 columns")


@pytest.mark.parametrize("strokes,bodies", [(65, 5), (129, 5), (128, 65)])
def test_the_body_at_a_time_helper_equals_the_model(strokes, bodies):
    same_brush(F.rows_answer(strokes, bodies), F.brush_model(*F.list_rows(strokes, bodies)), f"{strokes} strokes, {bodies} bodies")


@pytest.mark.parametrize("bodies", F.ROW_BODIES)
@pytest.mark.parametrize("strokes", F.ROW_STROKES)
def test_list_rows(brush_rules, tmp_path, strokes, bodies):
    print(f"C2 ({strokes} strokes, {bodies} bodies): {F.assert_list_rows(strokes, bodies)}")
    same_brush(run_brushes(brush_rules, tmp_path, [F.list_rows(strokes, bodies)])[0], F.rows_answer(strokes, bodies), f"{strokes} strokes, {bodies} bodies")


def test_chunk_edges(brush_rules, tmp_path):
    print(f"C3: {F.assert_chunk_edges()}")
    same_brush(run_brushes(brush_rules, tmp_path, [F.chunk_edges()])[0], F.edges_answer(), "eight models at the chunk edges")


def test_wide_sums(brush_rules, tmp_path):
    print(f"C4: {F.assert_wide_sums()}")
    same_brush(run_brushes(brush_rules, tmp_path, [F.wide_sums()])[0], F.wide_answer(), "a model 66000 long")


def test_brushes_at_the_coordinate_limit(brush_rules, tmp_path):
    cases = F.limit_brushes()
    print(f"D2: left out {F.assert_limit_brushes(cases)}")
    got = run_brushes(brush_rules, tmp_path, [at_limit for _, _, at_limit, _ in cases])
    for (name, origin, at_limit, delta), g in zip(cases, got):
        want = F.brush_model(*origin)
        assert want[3]["carved"] > 0 and want[2]["carved"].sum() > 0, name
        same_brush(F.brush_model(*at_limit), want, name + ": the answer at the origin")
        same_brush(g, want, name)
    for name in F.LIMIT_BRUSH_CASES:  # the strokes of the case at home do what they did there: the added sphere only carves
        home = modelbrushcases.answer(name)[1]
        for case in cases:
            if case[0].startswith(name + ":"):
                assert F.brush_model(*case[1])[1]["carved"][0] >= home["carved"][0] > 0


# ---- F. the flight loop ------------------------------------------------------------------------------------------------------------------------------

ORDER = ("slab", "pyramid", "ball")


def test_the_flight_brush_reaches_every_piece_and_is_seen_by_the_calls_after_it(brush_rules, tmp_path_factory, tmp_path):
    """On the host: the brush of the flight loop through the rules program and the model; then the five read-only calls' references for the
    bodies before and after it differ in a sweep, a pair and a pixel."""
    pieces = L.flight_world()[3]
    models = [(pieces[name][2], pieces[name][3]) for name in ORDER]
    chosen, strokes = F.flight_brush(ORDER)
    assert sorted(i.model for i in chosen) == [0, 1, 2] and len(strokes) == 4
    want = F.brush_model(models, chosen, strokes)
    after, results, hit, summary = want
    assert (results["carved"] > 0).all() and results["painted"][ORDER.index("ball")] > 0 and (hit["carved"] > 0).all() and summary["models"] == 3
    same_brush(run_brushes(brush_rules, tmp_path, [(models, chosen, strokes)])[0], want, "the flight brush")
    again = F.brush_model(after, chosen, strokes)
    assert again[3]["carved"] == 0 and all((again[1][name] == results[name]).all() for name in ("voxels", "sum", "moment", "min", "max")), "the same brush again carves nothing"
    pick_rules = ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("flight_pick"))
    draw_rules = ruleslib.build("model_draw_rules", tmp_path_factory.mktemp("flight_draw"))
    before = F.flight_references(models, ORDER, pick_rules, draw_rules, tmp_path)
    behind = F.flight_references(after, ORDER, pick_rules, draw_rules, tmp_path)
    F.assert_the_brush_is_seen(before, behind)
