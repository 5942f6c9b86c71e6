"""CPU (no GPU needed): the rules behind cvxc_world_contacts / cvxc_contact_response (cpuvox_amd/csrc/cvx_contacts.h), compiled for the host
through tests/contacts_rules.cpp, against the independent numpy model of tests/contactsmodel.py.  The program runs the scalar specification
(cvxb::ContactsInstance) AND the kernels' walk (a wave per pair, 64 lanes a step, the pair's sums added as the atomics add them) and fails when
they differ in a byte; its output must equal the model's bytes.  Everything is integers: no comparison has a tolerance.

- Random small worlds (seed 20260) under rotations, a mirror, scale 2 and 1/2, with boxes that stick out of the world on every side, boxes
  hundreds of voxels taller than their body (the walk cuts their step range) and every solidOutside bit; what the cases have to cover is asserted from the model first.
- Known answers: a 4 x 4 x 4 cube over, in and under flat ground, against a wall corner and below the world.
- The mixed call of tests/test_world_models_cpu.py on the terrain and the tall world.
- overlap = voxels - what a FILL of the instance newly makes solid (tests/modelsmodel.py's place).
- Every argument check with its message, cvxc_contact_response against the formula in Python float64, the wrappers' array checks.
- The same stand-alone program built with -fsanitize=address,undefined (the header's mirrors: tests/test_abi_contacts.py)."""
import subprocess

import numpy as np
import pytest

import contactsmodel
import modelsmodel
import pyworld
import ruleslib
from cpuvox_amd import gpu
from test_world_brush_cpu import _random_column
from test_world_models_cpu import ONE, as_dicts, build_world, call_words, forward_about_centre, identity_at, mixed_call, random_model, rotation, tilt

FLAT = (16, 32, 16)  # the hand-made worlds: ground solid for y < 8
CUBE = (4, 4, 4)
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("contacts_rules", tmp_path_factory.mktemp("contacts"))


# ---- building cases (the GPU test uses these too) -----------------------------------------------------------------------------------------------

def volume_columns(solid, colour):
    """The columns of a case world (tests/rules_world.h) that hold the (x, y, z) volume, encoded by the builder's rule."""
    columns = []
    for x in range(solid.shape[0]):
        for z in range(solid.shape[2]):
            ys = np.nonzero(solid[x, :, z])[0][::-1]
            col = pyworld.final_column([(int(y), int(colour[x, y, z])) for y in ys], solid.shape[1] - 1, 1)
            runs, colours = (col[0], col[1]) if col is not None else ([], [])
            columns.append((32 + len(columns) * 1000, list(runs), list(colours)))
    return columns


def colour_of(solid):
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.uint32) for n in solid.shape], indexing="ij")
    return np.where(solid, np.uint32(0xFF000000) | (x << 16) | (y << 8) | z, 0).astype(np.uint32)


def flat_world(wall=False, dims=FLAT):
    solid = np.zeros(dims, dtype=bool)
    solid[:, :8, :] = True
    if wall:  # a wall along x < 6, up to y = 20
        solid[:6, :20, :] = True
    return solid, colour_of(solid)


def cube_model():
    return (np.full((CUBE[0], CUBE[2], CUBE[1]), 0xFF112233, dtype=np.uint32), None)


def case_words(solid, colour, stride, models, instances, solid_outside, columns=None):
    dims = solid.shape
    return [ruleslib.world_words(dims[1], dims[0], dims[2], stride, columns if columns is not None else volume_columns(solid, colour)), call_words(models, instances),
            [solid_outside]]


def parse(raw, counts):
    """The bytes contacts_rules writes for cases of `counts` instances -> [(results, points, summary dict)]."""
    out, at = [], 0
    for n in counts:
        results = np.frombuffer(raw[at:at + 120 * n], dtype=contactsmodel.RESULT_DTYPE)
        at += 120 * n
        summary = dict(zip(contactsmodel.SUMMARY_NAMES, (int(v) for v in np.frombuffer(raw[at:at + 32], dtype=np.int64))))
        at += 32
        points = np.frombuffer(raw[at:at + 24 * summary["points"]], dtype=contactsmodel.POINT_DTYPE)
        at += 24 * summary["points"]
        out.append((results, points, summary))
    assert at == len(raw)
    return out


def same(got, want, what=""):
    """Results, points and summary byte for byte."""
    (r, p, s), (mr, mp, ms) = got, want
    for name in contactsmodel.RESULT_DTYPE.names:
        assert (np.asarray(r[name]) == mr[name]).all(), f"{what}: results differ in `{name}`: {r[name].tolist()} vs the model's {mr[name].tolist()}"
    assert r.tobytes() == mr.tobytes(), what
    assert s == ms, f"{what}: summary {s} vs the model's {ms}"
    assert len(p) == len(mp) and p.tobytes() == mp.tobytes(), f"{what}: the points differ"


def run_cases(rules, tmp_path, cases):
    """cases: [(solid, colour, stride, models, instances, solid_outside[, columns])] -> the program's parsed output."""
    parts = []
    for case in cases:
        parts += case_words(*case)
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *parts, dtype=np.uint8).tobytes()
    return parse(raw, [len(case[4]) for case in cases])


def check_against_model(rules, tmp_path, cases):
    got = run_cases(rules, tmp_path, cases)
    want = [contactsmodel.contacts(c[0], c[1], c[3], as_dicts(c[4]), c[5]) for c in cases]
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"case {k}")
    return want


# ---- random small worlds ------------------------------------------------------------------------------------------------------------------------

MAPS = {
    "yaw 45": rotation(1, 45), "tilt": tilt(), "quarter": rotation(1, 90), "roll 90": rotation(0, 90), "mirror": np.diag([1.0, 1.0, -1.0]), "scale 2": 2 * rotation(1, 30), "scale 1/2": 0.5 * np.eye(3),
}


def test_both_forms_match_the_model_on_random_small_worlds(rules, tmp_path):
    rng = np.random.default_rng(20260)
    cases = []
    names = sorted(MAPS)
    for n in range(240):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        gx, gz = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        solid = np.zeros((gx, dim_y, gz), dtype=bool)
        colour = np.zeros((gx, dim_y, gz), dtype=np.uint32)
        columns = []
        for k in range(gx * gz):
            runs, colours, column_solid, dense = _random_column(rng, dim_y)
            solid[k // gz, :, k % gz], colour[k // gz, :, k % gz] = column_solid, dense
            columns.append((32 + k * 20000 + int(rng.integers(0, 100)), runs, colours))
        colour[~solid] = 0
        models = [random_model(rng, (3, 5, 4), with_mask=bool(n % 2), zeros=0.2), random_model(rng, (2, 70, 2), zeros=0.1)]
        if n % 3 == 0:
            models[0] = (None, models[0][1] if models[0][1] is not None else models[0][0] != 0)  # a model without argb
        instances = []
        for _ in range(int(rng.integers(1, 4))):
            model = int(rng.integers(0, 2))
            name = names[int(rng.integers(0, len(names)))]
            size = (3, 5, 4) if model == 0 else (2, 70, 2)
            centre = (rng.uniform(-1, gx + 1), rng.uniform(-3, dim_y + 3), rng.uniform(-1, gz + 1))
            inst = gpu.model_instance(forward_about_centre(MAPS[name], size, centre), size, model, int(rng.integers(0, 4)))
            if rng.random() < 0.3:  # a box far taller than the body: more than the four steps a wave walks without cutting its range
                inst.boxMin[1] -= int(rng.integers(0, 400))
                inst.boxMax[1] += int(rng.integers(100, 400))
            instances.append((name, inst))
        cases.append((solid, colour, int(rng.choice([1, 32])), models, [i for _, i in instances], int(rng.integers(0, 64)), columns, [m for m, _ in instances]))
    want = [contactsmodel.contacts(c[0], c[1], c[3], as_dicts(c[4]), c[5]) for c in cases]
    # what the cases cover, from the model
    below, beyond = np.zeros(3, dtype=int), np.zeros(3, dtype=int)
    outside_overlap = np.zeros(6, dtype=int)  # overlap voxels beyond face f of the world
    touching = {name: 0 for name in names}
    bits = 0
    two_axes = with_points = buried = seams = tall_boxes = 0
    for case, (results, points, summary) in zip(cases, want):
        dims = case[0].shape
        bits |= case[5]
        for name, inst, r in zip(case[7], as_dicts(case[4]), results):
            for a in range(3):
                below[a] += inst["box_min"][a] < 0
                beyond[a] += inst["box_max"][a] > dims[a]
                if r["overlap"] > 0:
                    outside_overlap[2 * a] += r["min"][a] < 0
                    outside_overlap[2 * a + 1] += r["max"][a] > dims[a]
            touching[name] += r["overlap"] > 0
            two_axes += int((r["normal"] != 0).sum() >= 2)
            buried += r["overlap"] > 0 and r["points"] < r["overlap"]
            seams += inst["box_max"][1] - inst["box_min"][1] > 64 and r["overlap"] > 0
            tall_boxes += inst["box_max"][1] - inst["box_min"][1] > 4 * 64 + 64 and r["overlap"] > 0 and name in ("quarter", "roll 90", "tilt", "scale 2")
        with_points += summary["points"] > 0
    assert bits == 0x3F and (below > 10).all() and (beyond > 10).all(), "boxes stick out of the world on every side, every solidOutside bit is used"
    assert (outside_overlap > 0).all(), f"some overlap lies beyond every face of the world: {outside_overlap}"
    assert all(v > 5 for v in touching.values()), touching
    assert two_axes > 20 and with_points > 100 and buried > 20 and seams > 10 and tall_boxes > 10
    got = run_cases(rules, tmp_path, [c[:7] for c in cases])
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"case {k}")


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------

def _cube_at(at):
    return identity_at(at, CUBE, 0, gpu.BRUSH_FILL)


def test_known_answers_on_flat_ground(rules, tmp_path):
    solid, colour = flat_world()
    models = [cube_model()]
    cases = {
        "bottom layer": _cube_at((6, 7, 6)), "two layers": _cube_at((6, 6, 6)), "in air": _cube_at((6, 12, 6)), "buried": _cube_at((6, 2, 6)),
    }
    want = check_against_model(rules, tmp_path, [(solid, colour, 1, models, [inst], gpu.SURFACE_OUTSIDE_DEFAULT) for inst in cases.values()])
    answers = {name: w for name, w in zip(cases, want)}
    r, p, s = answers["bottom layer"]
    assert (r["voxels"][0], r["overlap"][0], r["points"][0], r["firstPoint"][0]) == (64, 16, 16, 0)
    assert r["normal"][0].tolist() == [0, 16, 0] and r["sum"][0].tolist() == [24, 0, 24] and r["origin"][0].tolist() == [6, 7, 6]
    assert r["min"][0].tolist() == [6, 7, 6] and r["max"][0].tolist() == [10, 8, 10] and r["pad_"][0] == 0
    assert len(p) == 16 and (p["faces"] == 0x08).all() and (p["voxel"][:, 1] == 7).all() and (p["instance"] == 0).all()
    assert p["voxel"][:, [0, 2]].tolist() == [[x, z] for x in range(6, 10) for z in range(6, 10)] and (p["argb"] == colour[p["voxel"][:, 0], 7, p["voxel"][:, 2]]).all()
    assert s == dict(touching=1, overlap=16, points=16, voxels=64)
    assert gpu.contact_response(r[0])[2] == 1.0 and gpu.contact_response(r[0])[1].tolist() == [0.0, 1.0, 0.0]
    assert gpu.contact_response(r[0])[0].tolist() == [8.0, 7.5, 8.0]
    r, p, s = answers["two layers"]
    assert (r["voxels"][0], r["overlap"][0], r["points"][0]) == (64, 32, 16) and r["normal"][0].tolist() == [0, 16, 0] and gpu.contact_response(r[0])[2] == 2.0
    assert (p["voxel"][:, 1] == 7).all() and r["min"][0].tolist() == [6, 6, 6] and r["max"][0].tolist() == [10, 8, 10]
    r, p, s = answers["in air"]
    assert r["voxels"][0] == 64 and s == dict(touching=0, overlap=0, points=0, voxels=64) and len(p) == 0
    assert not r["sum"][0].any() and not r["normal"][0].any() and not r["min"][0].any() and not r["max"][0].any() and r["origin"][0].tolist() == [6, 12, 6]
    r, p, s = answers["buried"]
    assert (r["voxels"][0], r["overlap"][0], r["points"][0]) == (64, 64, 0) and not r["normal"][0].any() and len(p) == 0
    assert r["min"][0].tolist() == [6, 2, 6] and r["max"][0].tolist() == [10, 6, 10]
    assert gpu.contact_response(r[0])[2] == 0.0 and not gpu.contact_response(r[0])[1].any()


def test_known_answers_at_a_wall_corner_and_below_the_world(rules, tmp_path):
    solid, colour = flat_world(wall=True)
    models = [cube_model()]
    corner = _cube_at((5, 7, 8))  # one layer in the wall, one in the ground
    under = _cube_at((8, -2, 8))  # two layers below y = 0, two in the ground
    edge = _cube_at((14, 7, 14))  # two columns beyond +X and +Z
    cases = [(solid, colour, 1, models, [corner], 0x04), (solid, colour, 1, models, [under], 0x04), (solid, colour, 1, models, [under], 0),
             (solid, colour, 32, models, [edge, corner], 0x02 | 0x20), (solid, colour, 32, models, [edge, corner], 0)]
    want = check_against_model(rules, tmp_path, cases)
    r = want[0][0][0]
    assert r["overlap"] == 16 + 12 and r["normal"].tolist() == [12, 12, 0], "a two-axis normal: 3 x 4 faces of the wall's layer, 3 x 4 of the ground's"
    assert set(want[0][1]["faces"].tolist()) == {0x02, 0x08}
    with_ground, without = want[1], want[2]
    assert with_ground[0]["overlap"][0] == 64 and with_ground[0]["points"][0] == 0 and not with_ground[0]["normal"][0].any()
    assert without[0]["overlap"][0] == 32 and without[0]["normal"][0].tolist() == [0, -16, 0] and (without[1]["faces"] == 0x04).all() and len(without[1]) == 16
    assert without[0]["min"][0].tolist() == [8, 0, 8] and with_ground[0]["min"][0].tolist() == [8, -2, 8]
    walled, open_ = want[3], want[4]
    assert open_[0]["overlap"][0] == 4 and walled[0]["overlap"][0] == 4 + 12 * 4, "the voxels beyond +X and +Z are solid only with their bits"
    assert (walled[1]["argb"][walled[1]["voxel"][:, 0] >= FLAT[0]] == 0).all() and (walled[1]["voxel"][:, 0] >= FLAT[0]).any(), "0 outside the world"
    assert walled[0]["firstPoint"][1] == walled[0]["points"][0] > 0
    # an instance's result does not depend on the other instances (but for firstPoint)
    alone = want[0][0][0].copy()
    for with_others in (walled[0][1], open_[0][1]):
        again = with_others.copy()
        again["firstPoint"] = 0
        assert again.tobytes() == alone.tobytes()


# ---- the worlds of the GPU tests ----------------------------------------------------------------------------------------------------------------

def run_world(rules, tmp_path, ws, models, instances, solid_outside):
    info = ws.info(0)
    blob, call, out = tmp_path / "world.bin", tmp_path / "call.bin", tmp_path / "contacts.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    call.write_bytes(np.concatenate([call_words(models, instances), np.int32([solid_outside])]).tobytes())
    subprocess.check_call([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(call), str(out)])
    return parse(out.read_bytes(), [len(instances)])[0]


@pytest.mark.parametrize("world_name", ["terrain", "tall"])
def test_the_mixed_call_matches_the_model(rules, tmp_path, world_name):
    from test_gpu_world_brush import _dense
    from test_gpu_world_dense import _tall_solid
    from test_gpu_world_edit import _terrain

    dims, solid = ((128, 64, 128), _terrain()) if world_name == "terrain" else ((32, 256, 32), _tall_solid())
    colour = _dense(solid)
    names, models, instances = mixed_call(np.random.default_rng(11), dims, gpu.BRUSH_FILL)
    want = contactsmodel.contacts(solid, colour, models, as_dicts(instances), gpu.SURFACE_OUTSIDE_DEFAULT)
    results = want[0]
    assert (results["overlap"] > 0).any() and (results["normal"] != 0).any() and (results["voxels"] > 0).all()
    d = as_dicts(instances)[names["partly outside"]]
    assert any(d["box_min"][a] < 0 or d["box_max"][a] > dims[a] for a in range(3))
    ws = build_world(dims, solid, colour)
    try:
        same(run_world(rules, tmp_path, ws, models, instances, gpu.SURFACE_OUTSIDE_DEFAULT), want, world_name)
    finally:
        ws.close()


def test_overlap_is_what_a_fill_would_overwrite():
    """For one instance inside the world: overlap = voxels - (voxels that modelsmodel.place FILL newly makes solid)."""
    from test_gpu_world_brush import _dense
    from test_gpu_world_edit import _terrain

    dims, solid = (128, 64, 128), _terrain()
    colour = _dense(solid)
    rng = np.random.default_rng(3)
    size = (9, 11, 7)
    model = random_model(rng, size, zeros=0.3)
    checked = 0
    for linear, (cx, cz) in ((rotation(1, 45), (40, 40)), (tilt(), (64, 90)), (2 * rotation(1, 30), (90, 30)), (0.5 * np.eye(3), (20, 100))):
        surface = int(np.nonzero(solid[cx, :, cz])[0].max())  # (the model straddles the terrain's surface)
        inst = gpu.model_instance(forward_about_centre(linear, size, (cx, surface, cz)), size, 0, gpu.BRUSH_FILL)
        d = as_dicts([inst])
        assert all(d[0]["box_min"][a] >= 0 and d[0]["box_max"][a] <= dims[a] for a in range(3)), "inside the world"
        results, _, _ = contactsmodel.contacts(solid, colour, [model], d, 0)
        filled, _ = modelsmodel.place(solid, colour, [model], d)
        newly = int((filled & ~solid).sum())
        assert 0 < newly < results["voxels"][0]
        assert results["overlap"][0] == results["voxels"][0] - newly
        checked += 1
    assert checked == 4


# ---- arguments, the helper, the wrappers --------------------------------------------------------------------------------------------------------

MESSAGES = [
    "models NULL or modelCount 1 outside 1 .. 256", "models NULL or modelCount 0 outside 1 .. 256", "models NULL or modelCount 257 outside 1 .. 256",
    "instances NULL or instanceCount 1 outside 1 .. 4096", "instances NULL or instanceCount 0 outside 1 .. 4096", "instances NULL or instanceCount 4097 outside 1 .. 4096",
    "model 0: size 0 on axis 1 is below 1", "model 0: 2^31 or more voxels", "model 0: argb and solid are both NULL", "instance 0: model 1 outside 0 .. 0",
    "instance 0: model -1 outside 0 .. 0", "instance 0: the box [0, 0) on axis 1 is empty", "instance 0: the box [0, 1073741825) on axis 2 has a coordinate beyond 2^30",
    "instance 0: the box [-1073741825, 2) on axis 0 has a coordinate beyond 2^30", "instance 0: toModel: m[1][2] = 16777217 beyond 2^24 (256 in units of 2^-16)",
    "instance 0: toModel: t[2] = -70368744177665 beyond 2^46 (2^30 in units of 2^-16)", "instance 3: the box [0, 0) on axis 1 is empty", "unknown solidOutside bits 0x40",
    "unknown solidOutside bits 0xffffffff", "results is NULL", "pointCapacity -1 with a list", "pointCapacity 2 with no list",
]


def _check_args(text):
    lines = text.splitlines()
    assert lines[:2] == ["-1", "-1"], "without a context"
    at = 2
    for message in MESSAGES:
        assert lines[at] == f"-1 cvxc_world_contacts: {message}" and lines[at + 1] == f"-1 cvxc_world_contacts_device: {message}", (lines[at], message)
        at += 2
    assert lines[at:at + 4] == ["-3 world LOD 0 has not been uploaded"] * 4, "valid arguments, no world yet"
    assert lines[at + 4] == "-4 cvxc_world_contacts: the boxes' footprints sum to 2^31 - 1 or more (instance, column) pairs"
    assert lines[at + 5] == "-4 cvxc_world_contacts_device: the boxes' footprints sum to 2^31 - 1 or more (instance, column) pairs"
    assert [line.strip() for line in lines[at + 6:]] == ["-1", "-1", "-1", "0"], "cvxc_contact_response"


def test_calls_fail_cleanly_with_their_messages(rules):
    _check_args(subprocess.check_output([rules, "args"], text=True))


def test_contact_response_is_the_formula(rules, tmp_path):
    """The helper's doubles equal the same formula in Python float64, bit for bit, on model results and on large hand-made sums."""
    solid, colour = flat_world(wall=True)
    rng = np.random.default_rng(9)
    model = random_model(rng, (5, 6, 4), zeros=0.2)
    instances = [gpu.model_instance(forward_about_centre(linear, (5, 6, 4), centre), (5, 6, 4), 0, gpu.BRUSH_FILL)
                 for linear, centre in ((rotation(1, 45), (6, 8, 8)), (tilt(), (9, 7, 5)), (rotation(2, 30), (3, 19, 12)), (np.eye(3), (8, 3, 8)))]
    results, _, _ = contactsmodel.contacts(solid, colour, [model], as_dicts(instances), gpu.SURFACE_OUTSIDE_DEFAULT)
    assert (results["overlap"] > 0).all() and len({tuple(r["normal"] != 0) for r in results}) >= 2
    big = np.zeros(3, dtype=contactsmodel.RESULT_DTYPE)
    big["overlap"] = [3, (1 << 53) + 1, 7]
    big["sum"] = [[(1 << 64) - 1, 10, 1 << 63], [12345678901234567, 3, 0], [1, 2, 4]]
    big["normal"] = [[-(1 << 40), 3, 1 << 62], [1, -1, 1], [0, 0, 0]]
    big["origin"] = [[-(1 << 30), 1 << 30, 7], [0, -5, 9], [1, 2, 3]]
    for r in list(results) + list(big):
        centre, normal, depth = gpu.contact_response(r)
        want_centre, want_normal, want_depth = contactsmodel.response(r)
        assert centre.tobytes() == want_centre.tobytes() and normal.tobytes() == want_normal.tobytes() and np.float64(depth).tobytes() == np.float64(want_depth).tobytes()
    assert gpu.contact_response(big[2])[2] == 0.0
    none = np.zeros(1, dtype=contactsmodel.RESULT_DTYPE)
    with pytest.raises(ValueError, match="no overlap"):
        gpu.contact_response(none[0])


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    inst = [identity_at((0, 0, 0), (2, 2, 2))]
    argb = np.zeros((2, 3, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="world_contacts: argb and solid are arrays of one shape"):
        gpu.Context.world_contacts(ctx, [(argb, np.zeros((2, 3, 5), dtype=bool))], inst)
    with pytest.raises(ValueError, match="world_contacts: a model is a pair"):
        gpu.Context.world_contacts(ctx, [argb], inst)
    with pytest.raises(ValueError, match="ModelInstance"):
        gpu.Context.world_contacts(ctx, [(argb, None)], [dict(op=0)])
    with pytest.raises(ValueError, match="world_contacts_device: a model is"):
        gpu.Context.world_contacts_device(ctx, [((2, 2), 0, 0)], inst, None)
    assert gpu.CONTACT_RESULT_DTYPE == contactsmodel.RESULT_DTYPE and gpu.CONTACT_POINT_DTYPE == contactsmodel.POINT_DTYPE
    assert gpu.CONTACTS_SUMMARY_DTYPE.names == contactsmodel.SUMMARY_NAMES and ONE == 65536


# ---- the sanitizer build ------------------------------------------------------------------------------------------------------------------------

def test_the_rules_run_clean_under_the_sanitizers(rules, tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python) built with -fsanitize=address,undefined: the argument checks and
    cases with boxes beyond every face of the world run to the end and give the bytes of the plain build."""
    program = ruleslib.build("contacts_rules", tmp_path, *SANITIZE)
    _check_args(subprocess.check_output([program, "args"], text=True))
    solid, colour = flat_world(wall=True)
    rng = np.random.default_rng(5)
    models = [cube_model(), random_model(rng, (2, 70, 2), with_mask=True, zeros=0.1)]
    instances = [_cube_at((-2, -2, -2)), _cube_at((14, 30, 14)), _cube_at((5, 7, 8)),
                 gpu.model_instance(forward_about_centre(tilt(), (2, 70, 2), (8, 16, 8)), (2, 70, 2), 1, gpu.BRUSH_FILL),
                 gpu.model_instance(forward_about_centre(2 * rotation(1, 30), CUBE, (15, 8, 0)), CUBE, 0, gpu.BRUSH_FILL)]
    cases = [(solid, colour, stride, models, instances, so) for stride, so in ((1, 0x3F), (32, 0), (32, 0x15))]
    plain, clean = tmp_path / "plain", tmp_path / "clean"
    plain.mkdir()
    clean.mkdir()
    want = [contactsmodel.contacts(c[0], c[1], c[3], as_dicts(c[4]), c[5]) for c in cases]
    assert all(w[2]["touching"] >= 2 for w in want)
    for g, w in zip(run_cases(program, clean, cases), want):
        same(g, w, "the sanitizer build")
    for g, w in zip(run_cases(rules, plain, cases), want):
        same(g, w, "the plain build")
