"""CPU (no GPU needed): the rules behind cvxs_world_sweep / cvxs_sweep_offset / cvxs_instance_moved (cpuvox_amd/csrc/cvx_sweep.h), compiled for
the host through tests/sweep_rules.cpp, against the independent numpy model of tests/sweepmodel.py.  The program runs the rule a pose at a time
(cvxb::SweepInstance over cvxb::ContactsInstance's own overlap) AND the kernel's walk (a wave per (instance, column, station) job, 64 lanes a
step, the minimum) and fails when they differ; its output must equal the model's bytes.  Everything is integers: no comparison has a tolerance.

- The path: the closed form equals the merge loop, and both the model's sorted fractions, for every motion with |v_a| <= 6 and three long ones;
  o_n = v, unit steps, the tie order; the stations against the path.
- cvxs_instance_moved: the body of I + o is the body of I shifted, under five maps; results beyond the limits are rejected.
- Rule, wave form and model agree byte for byte on every case of tests/sweepcases.py, the GPU test's; each case first asserts from the model
  the property it is named for.
- Every argument check with its message, the wrappers' array checks.
- The same stand-alone program built with -fsanitize=address,undefined (the header's mirrors: tests/test_abi_sweep.py)."""
import itertools
import subprocess

import numpy as np
import pytest

import contactsmodel
import ruleslib
import sweepcases
import sweepmodel
from cpuvox_amd import gpu
from test_world_contacts_cpu import case_words, flat_world
from test_world_models_cpu import as_dicts, build_world, call_words, forward_about_centre, identity_at, random_model, rotation, tilt

SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
LONG = [(4096, -4096, 4096), (4096, 1, 0), (1, 4096, 4095)]


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("sweep_rules", tmp_path_factory.mktemp("sweep"))


# ---- the path -----------------------------------------------------------------------------------------------------------------------------------------

def _paths(rules, tmp_path, motions):
    """sweep_rules path -> per motion (the merge loop's [(o, axis)], the closed form's, the stations as rows of ox oz j0 dy0 dyCount)."""
    raw = ruleslib.run_cases(rules, "path", tmp_path, np.asarray(motions).ravel(), dtype=np.int32)
    out, at = [], 0
    for v in motions:
        n = int(raw[at])
        assert n == sum(abs(c) for c in v)
        rows = raw[at + 1:at + 1 + 8 * (n + 1)].reshape(n + 1, 8)
        at += 1 + 8 * (n + 1)
        count = abs(v[0]) + abs(v[2]) + 1
        stations = raw[at:at + 5 * count].reshape(count, 5)
        at += 5 * count
        out.append(([(tuple(r[:3].tolist()), int(r[3])) for r in rows], [(tuple(r[4:7].tolist()), int(r[7])) for r in rows], stations))
    assert at == len(raw)
    return out


def _stations_of(path, v):
    """The stations from the model's path: a new one at every horizontal step."""
    rows = [[0, 0, 0, 0, 0]]
    for j, (o, axis) in enumerate(path[1:], start=1):
        if axis == 1:
            rows[-1][4] += 1
        else:
            rows.append([o[0], o[2], j, o[1], 0])
    return np.asarray(rows, dtype=np.int32)


def test_the_closed_form_is_the_merge_loop_and_the_model(rules, tmp_path):
    motions = list(itertools.product(range(-6, 7), repeat=3)) + LONG
    assert len(motions) == 2197 + 3
    for v, (merge, closed, stations) in zip(motions, _paths(rules, tmp_path, motions)):
        want = sweepmodel.path(v)
        assert merge == want, v
        assert closed == want, v
        assert merge[-1][0] == tuple(v) and merge[0] == ((0, 0, 0), -1)
        for (a, _), (b, axis) in zip(merge, merge[1:]):
            step = np.subtract(b, a)
            assert np.abs(step).sum() == 1 and step[axis] == np.sign(v[axis]), "one unit on one axis, with the motion's sign"
        assert (stations == _stations_of(want, v)).all(), v
        assert stations[:, 4].sum() == abs(v[1]) and len(stations) == abs(v[0]) + abs(v[2]) + 1


def test_the_tie_order_is_x_then_y_then_z():
    assert [a for _, a in sweepmodel.path((1, 1, 1))] == [-1, 0, 1, 2]
    assert [a for _, a in sweepmodel.path((2, 2, 2))] == [-1, 0, 1, 2, 0, 1, 2]
    assert [a for _, a in sweepmodel.path((-1, 1, -1))] == [-1, 0, 1, 2], "whatever the signs"
    for v in ((1, 1, 1), (2, 2, 2), (-2, 2, -2), (3, -1, 2)):
        want = sweepmodel.path(v)
        assert [gpu.sweep_offset(v, j) for j in range(len(want))] == [(list(o), a) for o, a in want]
    assert gpu.sweep_offset((3, -1, 2), 3) == ([2, 0, 1], 0) and gpu.sweep_offset((3, -1, 2), 4) == ([2, -1, 1], 1), "x before y at parameter 1/2"
    for j in (-1, 7):
        with pytest.raises(ValueError, match="outside 0 .. 6"):
            gpu.sweep_offset((3, -1, 2), j)
    with pytest.raises(ValueError, match="at most 4096"):
        gpu.sweep_offset((4097, 0, 0), 0)
    assert gpu.sweep_offset((4096, -4096, 4096), 12288) == ([4096, -4096, 4096], 2)


# ---- the moved instance -------------------------------------------------------------------------------------------------------------------------------

MOVED_MAPS = {"identity": np.eye(3), "yaw 30": rotation(1, 30), "tilt": tilt(), "scale 2": 2 * rotation(1, 30), "scale 1/2": 0.5 * np.eye(3)}


@pytest.mark.parametrize("name", sorted(MOVED_MAPS))
def test_the_moved_body_is_the_shifted_body(name):
    size = (5, 7, 4)
    model = random_model(np.random.default_rng(4), size, zeros=0.3)
    inst = gpu.model_instance(forward_about_centre(MOVED_MAPS[name], size, (3.25, -2.5, 9.75)), size, 0, gpu.BRUSH_FILL)
    body = contactsmodel.body([model], as_dicts([inst])[0])
    assert body.any()
    for o in ((1, 0, 0), (0, -1, 0), (0, 0, 1), (-7, 12, 5), (4096, -4096, 4096), (-100000, 3, 1 << 20)):
        there = gpu.instance_moved(inst, o)
        d = as_dicts([there])[0]
        assert d == sweepmodel.moved(as_dicts([inst])[0], o), "the model's own I + o"
        assert d["box_min"] == [inst.boxMin[a] + o[a] for a in range(3)] and d["model"] == inst.model and d["op"] == inst.op
        assert (contactsmodel.body([model], d) == body).all(), f"{name}: moved by {o}"


def test_instance_moved_rejects_results_beyond_the_limits():
    inst = identity_at((0, 0, 0), (2, 2, 2))
    edge = (1 << 30) - 2
    assert list(gpu.instance_moved(inst, (edge, -(1 << 30), 0)).boxMax) == [1 << 30, 2 - (1 << 30), 2]
    for o in ((edge + 1, 0, 0), (0, -(1 << 30) - 1, 0)):
        with pytest.raises(ValueError, match="leaves the limits"):
            gpu.instance_moved(inst, o)
    far = identity_at(((1 << 30) - 4, 0, 0), (2, 2, 2))  # t = -(2^30 - 4) * 65536: five more voxels pass 2^46
    assert gpu.instance_moved(far, (-6, 0, 0)).toModel.t[0] == -((1 << 30) - 10) * 65536
    big = gpu.model_instance(forward_about_centre(0.5 * np.eye(3), (2, 2, 2), ((1 << 29) - 8, 0, 0)), (2, 2, 2))  # m = 2: t doubles
    with pytest.raises(ValueError, match="leaves the limits"):
        gpu.instance_moved(big, (1 << 29, 0, 0))
    with pytest.raises(ValueError, match="three int32"):
        gpu.instance_moved(inst, (1 << 31, 0, 0))


# ---- rule, wave form and model on the GPU test's cases ---------------------------------------------------------------------------------------------------

def parse(raw, n):
    """The bytes sweep_rules writes for one call of n instances -> (sweeps, contacts, points, summary dict)."""
    sweeps = np.frombuffer(raw[:48 * n], dtype=sweepmodel.RESULT_DTYPE)
    at = 48 * n
    summary = dict(zip(sweepmodel.SUMMARY_NAMES, (int(v) for v in np.frombuffer(raw[at:at + 32], dtype=np.int64))))
    at += 32
    contacts = np.frombuffer(raw[at:at + 120 * n], dtype=contactsmodel.RESULT_DTYPE)
    at += 120 * n
    points = np.frombuffer(raw[at:], dtype=contactsmodel.POINT_DTYPE)
    assert len(points) == summary["points"]
    return sweeps, contacts, points, summary


def same(got, want, what=""):
    """Sweeps, contacts, points and summary byte for byte."""
    (s, c, p, t), (ms, mc, mp, mt) = got, want
    for name in sweepmodel.RESULT_DTYPE.names:
        assert (np.asarray(s[name]) == ms[name]).all(), f"{what}: sweeps differ in `{name}`: {np.asarray(s[name]).tolist()[:8]} vs the model's {ms[name].tolist()[:8]}"
    assert s.tobytes() == ms.tobytes(), what
    for name in contactsmodel.RESULT_DTYPE.names:
        assert (np.asarray(c[name]) == mc[name]).all(), f"{what}: contacts differ in `{name}`"
    assert c.tobytes() == mc.tobytes(), what
    assert t == mt, f"{what}: summary {t} vs the model's {mt}"
    assert len(p) == len(mp) and p.tobytes() == mp.tobytes(), f"{what}: the points differ"


def run_world(rules, tmp_path, key, models, instances, motions, solid_outside):
    dims, solid, colour = sweepcases.world(key)
    ws = build_world(dims, solid, colour)
    try:
        info = ws.info(0)
        blob, call, out = tmp_path / "world.bin", tmp_path / "call.bin", tmp_path / "sweep.bin"
        blob.write_bytes(ws.storage(0).tobytes())
        call.write_bytes(np.concatenate([call_words(models, instances), np.int32([solid_outside]), np.asarray(motions, dtype=np.int32).ravel()]).tobytes())
        subprocess.check_call([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(call), str(out)])
        return parse(out.read_bytes(), len(instances))
    finally:
        ws.close()


def property_of(name):
    """What the case is named for, asserted from the model's answer alone (the GPU test asserts it too, before it runs the device)."""
    key, models, instances, motions, so = sweepcases.case(name)
    dims, solid, colour = sweepcases.world(key)
    sweeps, contacts, points, summary = sweepcases.answer(name)
    s = sweeps[0]
    ends = lambda k: contactsmodel.contacts(solid, colour, models, [sweepmodel.moved(as_dicts(instances)[k], o) for o in ((0, 0, 0), motions[k])], so)[0]["overlap"]  # noqa: E731
    if name == "thin shell":
        assert ends(0).tolist() == [0, 0], "no overlap at either end pose: the plate falls through the floor"
        assert (s["hit"], s["axis"], s["sign"], s["steps"]) == (5, 1, -1, 12) and s["free"].tolist() == [0, -4, 0] and s["at"].tolist() == [0, -5, 0]
        assert contacts["overlap"][0] == 64 and contacts["normal"][0].tolist() == [0, 0, 0], "the floor is a voxel thick: both of its faces are open"
    elif name == "starts solid":
        assert (s["hit"], s["axis"], s["sign"]) == (0, -1, 0) and not s["free"].any() and not s["at"].any() and summary["startsSolid"] == 1
    elif name == "hit at n":
        assert s["hit"] == s["steps"] == 5 and s["at"].tolist() == [0, -5, 0]
    elif name == "miss by one":
        assert (s["hit"], s["axis"], s["sign"]) == (-1, -1, 0) and s["free"].tolist() == s["at"].tolist() == [0, -4, 0] and contacts["overlap"][0] == 0
    elif name == "still":
        assert sweeps["steps"].tolist() == [0, 0] and sweeps["hit"].tolist() == [-1, 0] and not sweeps["at"].any()
    elif name in ("-x", "+x", "-y", "+y", "-z", "+z"):
        axis, sign = "xyz".index(name[1]), (1 if name[0] == "+" else -1)
        assert s["hit"] > 0 and (s["axis"], s["sign"]) == (axis, sign) and ends(0)[0] == 0
    elif name in ("+x open", "sideways open"):
        assert (sweeps["hit"] == -1).all() and summary["hits"] == 0
    elif name == "3 -1 2":
        assert (s["hit"], s["axis"]) == (3, 0) and sweepmodel.path(motions[0])[4][1] == 1, "x and y tie at 1/2: x goes first and meets the wall beyond +X"
        assert ends(0)[1] > 0
    elif name == "2 2 2":
        assert (s["hit"], s["axis"], s["sign"]) == (4, 0, 1), "all three axes tie: x is the first to leave the world"
    elif name == "-5 7 -3":
        assert (s["hit"], s["axis"], s["sign"]) == (7, 0, -1) and [a for _, a in sweepmodel.path(motions[0])[7:10]] == [0, 1, 2], "a three-way tie at 1/2"
    elif name == "below the world":
        assert not solid[27, :, 27].any() and s["hit"] == 6 + 1 and s["at"].tolist() == [0, -7, 0], "the body's lowest y + 1"
    elif name == "sideways":
        assert sweeps["hit"].tolist() == [5, 6] and sweeps["axis"].tolist() == [0, 2], "29 + 3 = 32 at the third x step; 29 + 3 = 32 at the third z step, x going first"
    elif name.startswith("column "):
        height = int(name.split()[1])
        assert instances[0].boxMax[1] - instances[0].boxMin[1] == height and s["hit"] == -motions[0][1] - 1
        assert contacts["overlap"][0] == 1 and contacts["min"][0][1] == instances[0].boxMin[1] + s["at"][1], "the only touching voxel is the lowest: the last step's"
        assert (height > 4 * 64) == (name == "column 300")
    elif name in ("lane 0", "lane 63"):
        assert contacts["voxels"][0] == 1 and s["hit"] == (70 if name == "lane 0" else 7)
    elif name == "comb":
        assert (np.diff(solid[5, :, 5].astype(int)) == 1).sum() == 40, "40 runs"
        assert (sweeps["hit"] == 2).all() and sweeps["sign"].tolist() == [-1, 1] * 40
    elif name == "maps":
        assert (sweeps["hit"] > 0).sum() >= 8 and (contacts["voxels"] > 0).all()
        assert len({int(v) for v in contacts["voxels"]}) >= 3, "scales 2 and 1/2 give other bodies"
    elif name in ("65 instances", "4096 instances"):
        assert len(instances) == int(name.split()[0]) and (sweeps["hit"] > 0).sum() > len(instances) // 4 and (sweeps["hit"] == -1).any()
        assert {0, 1, 2} <= set(sweeps["axis"][sweeps["hit"] > 0].tolist())
    elif name == "8193 stations":
        assert summary["jobs"] == 8193 and 0 < s["hit"] < 200 and s["steps"] == 8195
    else:
        raise AssertionError(f"no property for {name}")


def test_every_case_has_its_property():
    for name in sweepcases.CASES:
        property_of(name)


@pytest.mark.parametrize("name", sorted(sweepcases.CASES))
def test_rule_and_wave_form_match_the_model(rules, tmp_path, name):
    property_of(name)
    key, models, instances, motions, so = sweepcases.case(name)
    same(run_world(rules, tmp_path, key, models, instances, motions, so), sweepcases.answer(name), name)


def test_small_random_worlds_through_the_case_files(rules, tmp_path):
    """Hand-made columns (tests/rules_world.h's cases, both strides) with every solidOutside bit: bodies that start outside on every side."""
    rng = np.random.default_rng(20261)
    solid, colour = flat_world(wall=True)
    parts, wants, counts = [], [], []
    for n in range(24):
        models = [random_model(rng, (3, 5, 4), with_mask=bool(n % 2), zeros=0.2)]
        instances, motions = [], []
        for _ in range(3):
            linear = [np.eye(3), rotation(1, 45), tilt(), 2 * np.eye(3)][int(rng.integers(0, 4))]
            centre = (rng.uniform(-4, 20), rng.uniform(14, 34), rng.uniform(-4, 20))
            instances.append(gpu.model_instance(forward_about_centre(linear, (3, 5, 4), centre), (3, 5, 4), 0, gpu.BRUSH_FILL))
            motions.append([int(rng.integers(-9, 10)), int(rng.integers(-16, 6)), int(rng.integers(-9, 10))])
        so = int(rng.integers(0, 64))
        parts += case_words(solid, colour, [1, 32][n % 2], models, instances, so) + [np.asarray(motions).ravel()]
        wants.append(sweepmodel.sweep(solid, colour, models, as_dicts(instances), motions, so))
        wants[-1][3]["jobs"] = sweepmodel.jobs(as_dicts(instances), motions)
        counts.append(len(instances))
    hits = np.concatenate([w[0]["hit"] for w in wants])
    assert (hits > 0).sum() > 10 and (hits == 0).sum() > 10 and (hits == -1).sum() > 3, "a dozen bodies that move and then touch, a dozen that start in solid"
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *parts, dtype=np.uint8).tobytes()
    at = 0
    for k, (n, want) in enumerate(zip(counts, wants)):
        size = 48 * n + 32 + 120 * n + 24 * want[3]["points"]
        same(parse(raw[at:at + size], n), want, f"case {k}")
        at += size
    assert at == len(raw)


# ---- arguments and the wrappers -----------------------------------------------------------------------------------------------------------------------

MESSAGES = [
    "models NULL or modelCount 1 outside 1 .. 256", "instances NULL or instanceCount 4097 outside 1 .. 4096", "model 0: argb and solid are both NULL",
    "instance 0: the box [0, 0) on axis 1 is empty", "unknown solidOutside bits 0x40", "pointCapacity -1 with a list", "pointCapacity 2 with no list",
    "motions is NULL", "sweeps is NULL", "pointCapacity 2 without contacts", "instance 0: motion 4097 on axis 1 beyond 4096", "instance 1: motion -4097 on axis 2 beyond 4096",
    "instance 0: moved by (11, 0, 0) it leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)",
    "instance 0: moved by (0, 2, 0) it leaves the limits (a box coordinate beyond 2^30 or t beyond 2^46)",
]


def test_calls_fail_cleanly_with_their_messages(rules):
    lines = subprocess.check_output([rules, "args"], text=True).splitlines()
    assert lines[:2] == ["-1", "-1"], "without a context"
    at = 2
    for message in MESSAGES:
        assert lines[at] == f"-1 cvxs_world_sweep: {message}" and lines[at + 1] == f"-1 cvxs_world_sweep_device: {message}", (lines[at], message)
        at += 2
    assert lines[at:at + 4] == ["-3 world LOD 0 has not been uploaded"] * 4, "valid arguments (contacts NULL among them), no world yet"
    assert lines[at + 4] == "-4 cvxs_world_sweep: the boxes' footprints times their motions' stations sum to 2^31 - 1 or more jobs"
    assert lines[at + 5] == "-4 cvxs_world_sweep_device: the boxes' footprints times their motions' stations sum to 2^31 - 1 or more jobs"
    assert lines[at + 6:] == ["-1 -1 -1 -1 -1 -1 0", "-1 -1 -1 -1 -1 0"], "cvxs_sweep_offset, cvxs_instance_moved"


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    inst = [identity_at((0, 0, 0), (2, 2, 2))]
    argb = np.zeros((2, 3, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="world_sweep: a model is a pair"):
        gpu.Context.world_sweep(ctx, [argb], inst, [(0, 0, 0)])
    with pytest.raises(ValueError, match=r"world_sweep: motions is an integer array of shape \(instances, 3\)"):
        gpu.Context.world_sweep(ctx, [(argb, None)], inst, [(0, 0, 0), (1, 1, 1)])
    with pytest.raises(ValueError, match="world_sweep: motions is an integer array"):
        gpu.Context.world_sweep(ctx, [(argb, None)], inst, [(0.5, 0, 0)])
    with pytest.raises(ValueError, match="world_sweep_device: a model is"):
        gpu.Context.world_sweep_device(ctx, [((2, 2), 0, 0)], inst, [(0, 0, 0)])
    assert gpu.SWEEP_RESULT_DTYPE == sweepmodel.RESULT_DTYPE and gpu.SWEEPS_SUMMARY_DTYPE.names == sweepmodel.SUMMARY_NAMES
    assert gpu.SWEEP_MAX_MOTION == sweepmodel.MAX_MOTION == 4096


# ---- the sanitizer build ------------------------------------------------------------------------------------------------------------------------------

def test_the_rules_run_clean_under_the_sanitizers(rules, tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python, nothing of the library is linked) built with
    -fsanitize=address,undefined: the paths, the longest among them, and cases with bodies beyond every face of the world run to the end and give
    the bytes of the plain build."""
    program = ruleslib.build("sweep_rules", tmp_path, *SANITIZE, "-DSWEEP_RULES_NO_LIBRARY", link_library=False)
    motions = [(3, -1, 2), (0, 0, 0), (-6, 6, 5)] + LONG
    clean, plain = tmp_path / "clean", tmp_path / "plain"
    clean.mkdir()
    plain.mkdir()
    for (m0, c0, s0), (m1, c1, s1) in zip(_paths(program, clean, motions), _paths(rules, plain, motions)):
        assert m0 == m1 == c0 == c1 and (s0 == s1).all()
    solid, colour = flat_world(wall=True)
    models = [random_model(np.random.default_rng(5), (2, 70, 2), with_mask=True, zeros=0.1), (np.full((4, 4, 4), 0xFF112233, dtype=np.uint32), None)]
    instances = [identity_at((-2, -2, -2), (4, 4, 4), 1, 0), identity_at((14, 30, 14), (4, 4, 4), 1, 0), identity_at((9, 9, 8), (4, 4, 4), 1, 0),
                 gpu.model_instance(forward_about_centre(tilt(), (2, 70, 2), (8, 50, 8)), (2, 70, 2), 0, gpu.BRUSH_FILL)]
    motions = [(5, 5, 5), (-9, -30, 4), (-5, 7, -3), (3, -40, 2)]
    parts = []
    for stride, so in ((1, 0x3F), (32, 0), (32, 0x15)):
        parts += case_words(solid, colour, stride, models, instances, so) + [np.asarray(motions).ravel()]
    got = [ruleslib.run_cases(p, "cases", d, *parts, dtype=np.uint8).tobytes() for p, d in ((program, clean), (rules, plain))]
    assert got[0] == got[1] and len(got[0]) > 3 * (4 * 168 + 32)
    want = sweepmodel.sweep(solid, colour, models, as_dicts(instances), motions, 0x3F)
    assert (want[0]["hit"] >= 0).sum() >= 3
    same(parse(got[0][:4 * 168 + 32 + 24 * want[3]["points"]], 4), (*want[:3], dict(want[3], jobs=sweepmodel.jobs(as_dicts(instances), motions))), "the sanitizer build")
