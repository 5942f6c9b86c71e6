"""CPU (no GPU needed): the rules behind cvxm_pair_sweep (cpuvox_amd/csrc/cvx_pair_sweep.h), compiled for the host through
tests/pair_sweep_rules.cpp, against the independent numpy model of tests/pairsweepmodel.py.  The program runs the rule a pose at a time
(cvxb::PairSweepPair over cvxb::PairOf's own overlap) AND the kernel's walk (a wave per (pair, column) job, its 64 lanes run in turn, the
minimum) and fails when they differ; its output must equal the model's bytes.  Everything is integers: no comparison has a tolerance.

- Rule, wave form and model agree byte for byte on every case of tests/pairsweepcases.py, the GPU test's; each case first asserts from the model
  the property it is named for.  hit(a, b, v) == hit(b, a, -v) on the path cases, from the model.
- The job rule: the prefix against the header's R_c counted a coordinate at a time (in the program) and against the model.
- The windows' closed form against the merge loop for every motion of [-4, 4]^3 and four with a component of 4096.
- Every argument check with its message, for both entry points; the wrappers' array checks.
- The same stand-alone program built with -fsanitize=address,undefined."""
import itertools
import subprocess

import numpy as np
import pytest

import paircontactsmodel
import pairsweepcases
import pairsweepmodel
import ruleslib
import sweepmodel
from cpuvox_amd import gpu
from test_world_models_cpu import as_dicts, call_words, identity_at

SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
LONG = [(4096, -4096, 4096), (4096, 1, 0), (1, 4096, 4095), (-3, 2, -4096)]


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("pair_sweep_rules", tmp_path_factory.mktemp("pairsweep"))


def words_of(models, instances, pairs, motions):
    """One call as tests/pair_sweep_rules.cpp reads it."""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return np.concatenate([call_words(models, instances), np.int32([len(pairs)]), pairs.ravel(), np.asarray(motions, dtype=np.int32).ravel()])


def parse(raw, n):
    """The bytes pair_sweep_rules writes for one call of n pairs -> (sweeps, contacts, summary dict)."""
    sweeps = np.frombuffer(raw[:56 * n], dtype=pairsweepmodel.RESULT_DTYPE)
    words = np.frombuffer(raw[56 * n:56 * n + 32], dtype=np.int64)
    assert words[3] == 0, "the summary's pad word"
    contacts = np.frombuffer(raw[56 * n + 32:56 * n + 32 + 144 * n], dtype=paircontactsmodel.RESULT_DTYPE)
    return sweeps, contacts, dict(zip(pairsweepmodel.SUMMARY_NAMES, (int(v) for v in words[:3])))


def same(got, want, what=""):
    """Sweeps, contacts and summary byte for byte."""
    (s, c, t), (ms, mc, mt) = got, want
    for name in sweepmodel.RESULT_DTYPE.names:
        mine, theirs = np.asarray(s["sweep"][name]), ms["sweep"][name]
        assert (mine == theirs).all(), f"{what}: sweeps differ in `{name}`: {mine.tolist()[:8]} vs the model's {theirs.tolist()[:8]}"
    assert s.tobytes() == ms.tobytes(), what
    if mc is not None:
        for name in paircontactsmodel.RESULT_DTYPE.names:
            assert (np.asarray(c[name]) == mc[name]).all(), f"{what}: contacts differ in `{name}`"
        assert c.tobytes() == mc.tobytes(), what
    assert t == mt, f"{what}: summary {t} vs the model's {mt}"


# ---- rule, wave form and model on the GPU test's cases ------------------------------------------------------------------------------------------------

def test_every_case_has_its_property():
    for name in pairsweepcases.CASES:
        pairsweepcases.property_of(name)


@pytest.mark.parametrize("name", sorted(pairsweepcases.CASES))
def test_rule_and_wave_form_match_the_model(rules, tmp_path, name):
    pairsweepcases.property_of(name)
    models, instances, pairs, motions = pairsweepcases.case(name)
    raw = ruleslib.run_cases(rules, "cases", tmp_path, words_of(models, instances, pairs, motions), dtype=np.uint8).tobytes()
    assert len(raw) == (56 + 144) * len(pairs) + 32
    same(parse(raw, len(pairs)), pairsweepcases.answer(name), name)


@pytest.mark.parametrize("name", ["-x", "+x", "-y", "+y", "-z", "+z", *pairsweepcases.TIES, "maps", "fuzz"])
def test_the_hit_of_a_b_under_v_is_the_hit_of_b_a_under_minus_v(name):
    """A property of the definition, from the model alone: the path of -v is the path of v negated."""
    models, instances, pairs, motions = pairsweepcases.case(name)
    pairs, motions = np.asarray(pairs)[:60], np.asarray(motions)[:60]
    forth = pairsweepcases.answer(name)[0]["sweep"][:60]
    back = pairsweepmodel.sweep(models, as_dicts(instances), pairs[:, ::-1], -motions, want_contacts=False)[0]["sweep"]
    assert forth["hit"].tolist() == back["hit"].tolist() and forth["axis"].tolist() == back["axis"].tolist() and (forth["at"] == -back["at"]).all()
    assert (forth["hit"] > 0).any()


# ---- the job rule -------------------------------------------------------------------------------------------------------------------------------------

def test_the_job_rule():
    """|R_x| * |R_z| if R_y is not empty: by hand on one pair, and a pair without jobs has hit -1 in the model's own walk."""
    a, b = identity_at((0, 0, 0), (4, 3, 5), 0, 0), identity_at((6, 10, 2), (2, 2, 2), 0, 0)
    da, db = as_dicts([a, b])
    assert pairsweepmodel.pair_jobs(da, db, (0, 0, 0)) == 0, "apart on x and y"
    assert pairsweepmodel.pair_jobs(da, db, (3, 8, 0)) == 1 * 2, "x: only u = 3 reaches 6; y: u = 2 reaches 10; z stands still: u = 2, 3 lie in [2, 4)"
    assert pairsweepmodel.pair_jobs(da, db, (3, 7, 0)) == 0, "y: 2 + 7 = 9 stays below 10"
    assert pairsweepmodel.pair_jobs(da, db, (9, 12, -4)) == 4 * 3, "every x reaches [6, 8); z goes down: u = 2, 3, 4 start inside or above, u = 0, 1 below"
    assert pairsweepmodel.pair_jobs(db, da, (-9, -12, 4)) == 2 * 2, "the other way round it is the columns of the other box that are counted"
    for name in ("repeats", "windows", "boxes", "still", "64 pairs"):
        models, instances, pairs, motions = pairsweepcases.case(name)
        sweeps, _, summary = pairsweepcases.answer(name)
        dicts = as_dicts(instances)
        per_pair = [pairsweepmodel.pair_jobs(dicts[int(p[0])], dicts[int(p[1])], v) for p, v in zip(pairs, motions)]
        assert sum(per_pair) == summary["jobs"] == pairsweepmodel.jobs(dicts, pairs, motions)
        assert all(h == -1 for h, n in zip(sweeps["sweep"]["hit"], per_pair) if n == 0)


# ---- the windows --------------------------------------------------------------------------------------------------------------------------------------

def test_the_windows_closed_form_is_the_merge_loop(rules, tmp_path):
    motions = list(itertools.product(range(-4, 5), repeat=3)) + LONG
    assert len(motions) == 729 + 4
    out = ruleslib.run_cases(rules, "windows", tmp_path, np.asarray(motions).ravel(), dtype=np.int32).reshape(-1, 2)
    assert len(out) == len(motions)
    for v, (compared, held) in zip(motions, out):
        n = [abs(c) for c in v]
        if max(n) <= 4:
            assert compared == sum((2 * k + 3) * (2 * k + 4) // 2 for k in n) + 48, v
            assert held >= sum((k + 1) * (k + 2) // 2 for k in n), f"{v}: every interval inside the range holds a pose"
        else:
            assert compared > 3 * 30 and held > 40, v


# ---- arguments and the wrappers -----------------------------------------------------------------------------------------------------------------------

MESSAGES = [
    "models NULL or modelCount 1 outside 1 .. 256", "instances NULL or instanceCount 4097 outside 1 .. 4096", "model 0: argb and solid are both NULL",
    "instance 1: the box [0, 0) on axis 1 is empty", "pairs NULL or pairCount 1 outside 1 .. 65536", "pairs NULL or pairCount 0 outside 1 .. 65536",
    "pairs NULL or pairCount 65537 outside 1 .. 65536", "pair 2: (1, 2) has an index outside 0 .. 1", "pair 1: (1, 1) pairs an instance with itself",
    "motions is NULL", "sweeps is NULL", "pair 0: motion 4097 on axis 1 beyond 4096", "pair 1: motion -4097 on axis 2 beyond 4096",
    "pair 0: instance 1 moved by (11, 0, 0) leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)",
    "pair 0: instance 0 moved by (0, 2, 0) leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)",
]
TOO_MANY = "the columns of the moving bodies that can come over the other body sum to 2^31 - 1 or more jobs"


def test_calls_fail_cleanly_with_their_messages(rules):
    lines = subprocess.check_output([rules, "args"], text=True).splitlines()
    assert lines[:2] == ["-1", "-1"], "without a context"
    at = 2
    for message in MESSAGES:
        assert lines[at] == f"-1 cvxm_pair_sweep: {message}" and lines[at + 1] == f"-1 cvxm_pair_sweep_device: {message}", (lines[at], message)
        at += 2
    assert lines[at:at + 2] == [f"-4 cvxm_pair_sweep: {TOO_MANY}", f"-4 cvxm_pair_sweep_device: {TOO_MANY}"]
    assert lines[at + 2:] == ["1"], "body b may lie beside the edge: only I_a + v is checked"


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    inst = [identity_at((0, 0, 0), (2, 2, 2)), identity_at((4, 0, 0), (2, 2, 2))]
    argb = np.zeros((2, 3, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="model_sweep: a model is a pair"):
        gpu.Context.model_sweep(ctx, [argb], inst, [(0, 1)], [(0, 0, 0)])
    with pytest.raises(ValueError, match=r"model_sweep: motions is an integer array of shape \(pairs, 3\)"):
        gpu.Context.model_sweep(ctx, [(argb, None)], inst, [(0, 1)], [(0, 0, 0), (1, 1, 1)])
    with pytest.raises(ValueError, match="model_sweep: motions is an integer array"):
        gpu.Context.model_sweep(ctx, [(argb, None)], inst, [(0, 1)], [(0.5, 0, 0)])
    with pytest.raises(ValueError, match="model_sweep: pairs is an"):
        gpu.Context.model_sweep(ctx, [(argb, None)], inst, [0, 1], [(0, 0, 0)])
    with pytest.raises(ValueError, match="model_sweep_device: a model is"):
        gpu.Context.model_sweep_device(ctx, [((2, 2), 0, 0)], inst, [(0, 1)], [(0, 0, 0)])
    assert gpu.PAIR_SWEEP_RESULT_DTYPE == pairsweepmodel.RESULT_DTYPE and gpu.PAIR_SWEEPS_SUMMARY_DTYPE.names == pairsweepmodel.SUMMARY_NAMES + ("pad_",)
    assert gpu.PAIR_SWEEP_EXPORTS == ["cvxm_pair_sweep", "cvxm_pair_sweep_device"]


# ---- the sanitizer build ------------------------------------------------------------------------------------------------------------------------------

def test_the_rules_run_clean_under_the_sanitizers(rules, tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python, nothing of the library is linked) built with
    -fsanitize=address,undefined: windows, the longest motions among them, and cases with tall, rotated and cut bodies run to the end and give
    the bytes of the plain build."""
    program = ruleslib.build("pair_sweep_rules", tmp_path, *SANITIZE, "-DPAIR_SWEEP_RULES_NO_LIBRARY", link_library=False)
    clean, plain = tmp_path / "clean", tmp_path / "plain"
    clean.mkdir()
    plain.mkdir()
    motions = np.asarray([(3, -1, 2), (0, 0, 0), (-4, 4, 3)] + LONG).ravel()
    got = [ruleslib.run_cases(p, "windows", d, motions, dtype=np.int32) for p, d in ((program, clean), (rules, plain))]
    assert (got[0] == got[1]).all() and len(got[0]) == 2 * 7
    parts = [words_of(*pairsweepcases.case(name)) for name in ("maps", "boxes", "column 300", "later step", "windows", "long hit", "65 pairs")]
    raw = [ruleslib.run_cases(p, "cases", d, *parts, dtype=np.uint8).tobytes() for p, d in ((program, clean), (rules, plain))]
    assert raw[0] == raw[1] and len(raw[0]) == sum(200 * len(pairsweepcases.case(name)[2]) + 32 for name in ("maps", "boxes", "column 300", "later step", "windows", "long hit", "65 pairs"))
