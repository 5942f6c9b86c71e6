"""CPU (no GPU needed): the rules behind cvx_world_place_models / cvx_world_read_model (cpuvox_amd/csrc/cvx_models.h), compiled for the host
through tests/models_rules.cpp, against the independent numpy model of tests/modelsmodel.py, which applies the contract voxel by voxel to a
dense volume.  Everything is integers: every comparison is byte for byte.

- World mode: calls over the 128 x 64 x 128 terrain and the 32 x 256 x 32 tall world of tests/test_gpu_world_dense.py.  The program runs
  cvxb::ModelsColumn AND the kernels' walk (the cull, then cvx_dense.h's steps with cvxb::ModelsLaneVoxel, lane after lane) on every column of
  the rectangle and fails when they differ in a word; its sub-world blob must equal the region of the world the host builds from the model's
  volume.
- The identity map against cvxb::DenseColumn, the 16 quarter-turn / mirror / flip transforms against tests/copymodel.py.
- Column mode: the over-limit rejection on a synthetic 40000-voxel column.
- The read, the matrix helper, the argument checks and the wrappers' array checks (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import copymodel
import densemodel
import modelsmodel
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world
from test_world_dense_cpu import FILL, CARVE, PAINT, REPLACE, _builder_column, _compare, random_dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"fill": FILL, "carve": CARVE, "paint": PAINT, "replace": REPLACE}
DIMS, TALL = (128, 64, 128), (32, 256, 32)
ONE = 65536


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("models_rules", tmp_path_factory.mktemp("models"))


# ---- building calls (the GPU test uses these too) -----------------------------------------------------------------------------------------------

def make_instance(m, t, box_min, box_max, model=0, op=REPLACE):
    """A gpu.ModelInstance from integers in units of 2^-16."""
    inst = gpu.ModelInstance()
    for i in range(3):
        for j in range(3):
            inst.toModel.m[i][j] = int(m[i][j])
        inst.toModel.t[i] = int(t[i])
        inst.boxMin[i], inst.boxMax[i] = int(box_min[i]), int(box_max[i])
    inst.model, inst.op = model, op
    return inst


def identity_at(at, size, model=0, op=REPLACE):
    """The instance that places a model of `size` (sx, sy, sz) as it lies with its corner at `at`."""
    return make_instance(np.eye(3, dtype=np.int64) * ONE, [-int(a) * ONE for a in at], at, [at[i] + size[i] for i in range(3)], model, op)


def rotation(axis, degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


def forward_about_centre(linear, size, centre_at):
    """The 3 x 4 matrix that applies `linear` about the model's centre and puts that centre at `centre_at`."""
    linear = np.asarray(linear, dtype=np.float64)
    half = np.asarray(size, dtype=np.float64) / 2
    return np.concatenate([linear, (np.asarray(centre_at, dtype=np.float64) - linear @ half)[:, None]], axis=1)


def model_size(model):
    shape = (model[0] if model[0] is not None else model[1]).shape
    return (shape[0], shape[2], shape[1])


def random_model(rng, size, with_mask=False, zeros=0.3):
    """(argb, mask or None) for a model of `size` (sx, sy, sz); arrays are (X, Z, Y)."""
    return random_dense(rng, (size[0], size[2], size[1]), zeros=zeros, with_mask=with_mask)


def tilt():
    return rotation(0, 20) @ rotation(1, 35) @ rotation(2, -25)


def mixed_call(rng, dims, op):
    """The named instances of one call over a world of `dims`, every one with `op`: name -> index; the models; the instances.  A yaw of 45
    degrees, a tilt about all three axes, scales 1/2, 2 and 3, a negative determinant, a 1 x 1 x 1 model, a 5 x 70 x 3 model (taller than a
    wave), a box narrower than the mapped model and an instance partly outside the world.  CARVE uses mask-only models."""
    dx, dy, dz = dims
    mask_only = op == CARVE
    sizes = [(9, 11, 7), (1, 1, 1), (5, 70, 3), (6, 5, 8)]
    models = []
    for size in sizes:
        argb, mask = random_model(rng, size, with_mask=True)
        if size == (1, 1, 1):  # its one voxel is set
            argb[...], mask[...] = 0xFF778899, True
        models.append((None, mask) if mask_only else (argb, mask if size[0] == 6 else None))
    cy = 8  # (the models straddle the ground of both worlds: every op finds solid voxels and air)
    specs = {
        "yaw 45": (0, rotation(1, 45), (dx * 0.25, cy, dz * 0.25)),
        "tilt": (0, tilt(), (dx * 0.5, cy + 3, dz * 0.25)),
        "scale 1/2": (0, 0.5 * np.eye(3), (dx * 0.75, cy, dz * 0.25)),
        "scale 2": (3, 2 * rotation(1, 30), (dx * 0.25, cy, dz * 0.6)),
        "scale 3": (3, 3 * np.eye(3), (dx * 0.6, cy + 2, dz * 0.6)),
        "negative determinant": (0, rotation(1, 10) @ np.diag([1.0, 1.0, -1.0]), (dx * 0.85, cy, dz * 0.7)),
        "1 x 1 x 1": (1, 1.5 * rotation(2, 45), (dx * 0.4, 2.0, dz * 0.85)),
        "tall": (2, rotation(2, 8), (dx * 0.15, min(dy * 0.5, 60), dz * 0.85)),
        "partly outside": (0, rotation(1, 60) * 1.5, (dx - 2, dy - 3, 1)),
    }
    names, instances = {}, []
    for name, (model, linear, centre) in specs.items():
        names[name] = len(instances)
        instances.append(gpu.model_instance(forward_about_centre(linear, sizes[model], centre), sizes[model], model, op))
    # a box narrower than the mapped model: it clips
    narrow = gpu.model_instance(forward_about_centre(rotation(1, 45), sizes[0], (dx * 0.5, cy, dz * 0.85)), sizes[0], 0, op)
    names["narrow box"] = len(instances)
    narrow.boxMin[0] += 4
    narrow.boxMax[2] -= 5
    narrow.boxMax[1] -= 3
    instances.append(narrow)
    return names, models, instances


def call_words(models, instances):
    """One call as tests/models_rules.cpp reads it."""
    words = [np.int32([len(models)])]
    for argb, mask in models:
        size = model_size((argb, mask))
        words.append(np.int32(list(size) + [int(argb is not None), int(mask is not None)]))
        if argb is not None:
            words.append(np.ascontiguousarray(argb, dtype=np.uint32).ravel().view(np.int32))
        if mask is not None:
            words.append(np.ascontiguousarray(mask).ravel().astype(np.int32))
    words.append(np.int32([len(instances)]))
    for inst in instances:
        words.append(np.frombuffer(bytes(inst), dtype=np.int32))
    return np.concatenate(words)


def as_dicts(instances):
    return [modelsmodel.from_struct(i) for i in instances]


def build_world(dims, solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _run_world(rules, tmp_path, ws, models, instances, rect, dense=False):
    info = ws.info(0)
    blob, call, out = tmp_path / "world.bin", tmp_path / "call.bin", tmp_path / "sub.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    call.write_bytes(call_words(models, instances).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(call),
                                    *[str(v) for v in rect], str(out)] + (["dense"] if dense else []), text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) over (\d+)", text)
    assert int(m.group(3)) == 0
    return out.read_bytes()


def _expected_region(dims, solid, colour, rect):
    ws = build_world(dims, solid, colour)
    try:
        return ws.extract_region(0, *rect)[0]
    finally:
        ws.close()


@pytest.fixture(scope="module")
def worlds():
    from test_gpu_world_brush import _dense
    from test_gpu_world_dense import _tall_solid
    from test_gpu_world_edit import _terrain

    out = {}
    for name, dims, solid in (("terrain", DIMS, _terrain()), ("tall", TALL, _tall_solid())):
        colour = _dense(solid)
        out[name] = (dims, solid, colour, build_world(dims, solid, colour))
    yield out
    for entry in out.values():
        entry[3].close()


def _check_call(rules, tmp_path, world, models, instances, level_count, what, dense=False):
    """The program's sub-world blob of the call's rectangle against the model's world; returns the model's (solid, colour)."""
    dims, solid, colour, ws = world
    dicts = as_dicts(instances)
    rect = modelsmodel.rectangle(dicts, dims, level_count)
    s, c = modelsmodel.place(solid, colour, models, dicts)
    got = _run_world(rules, tmp_path, ws, models, instances, rect, dense)
    want = _expected_region(dims, s, c, rect)
    assert got == want, f"{what}: the sub-world blob of {rect} differs from the model's ({len(got)} vs {len(want)} bytes)"
    return s, c


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world_name", ["terrain", "tall"])
@pytest.mark.parametrize("op_name", sorted(OPS))
def test_rule_matches_the_model(rules, tmp_path, worlds, world_name, op_name):
    world = worlds[world_name]
    dims, solid, colour, _ = world
    op = OPS[op_name]
    names, models, instances = mixed_call(np.random.default_rng(7 + op), dims, op)
    dicts = as_dicts(instances)
    # every instance does what it is named for
    for name, k in names.items():
        s, c = modelsmodel.place(solid, colour, models, [dicts[k]])
        changed = (s != solid) | (c != colour)
        if not (op_name in ("paint", "carve") and name == "partly outside"):  # (the world's top corner is air: nothing to paint or carve)
            assert changed.any(), f"{name} changes nothing"
        m = np.array(dicts[k]["m"], dtype=np.float64) / ONE
        det = np.linalg.det(m)
        if name == "negative determinant":
            assert det < 0
        if name.startswith("scale"):
            assert abs(abs(det) ** (-1 / 3) - eval(name.split()[1])) < 1e-3  # noqa: S307  (the forward scale: "1/2", "2", "3")
        if name == "tall":
            assert model_size(models[dicts[k]["model"]])[1] == 70 > 64
        if name == "partly outside":
            assert any(dicts[k]["box_min"][i] < 0 or dicts[k]["box_max"][i] > dims[i] for i in range(3))
        if name == "narrow box":
            wide = dict(dicts[k], box_min=[dicts[k]["box_min"][0] - 4] + dicts[k]["box_min"][1:],
                        box_max=[dicts[k]["box_max"][0], dicts[k]["box_max"][1] + 3, dicts[k]["box_max"][2] + 5])
            s2, c2 = modelsmodel.place(solid, colour, models, [wide])
            if op_name != "paint":
                assert ((s2 != s) | (c2 != c)).any(), "the narrow box clips nothing"
    assert np.linalg.det(np.array(dicts[names["yaw 45"]]["m"], dtype=np.float64) / ONE) > 0
    s, c = _check_call(rules, tmp_path, world, models, instances, 3, f"{world_name}, {op_name}")
    assert ((s != solid) | (c != colour)).any()


def test_the_identity_map_is_the_dense_write(rules, tmp_path, worlds):
    """One instance with the identity map and its model's box: cvxb::ModelsColumn equals cvxb::DenseColumn of the same arrays and box word for
    word (the program compares them), and the model equals tests/densemodel.py's write."""
    for world_name, at in (("terrain", (30, 5, 40)), ("tall", (-3, 50, 7))):
        world = worlds[world_name]
        dims, solid, colour, _ = world
        rng = np.random.default_rng(3)
        for op in OPS.values():
            size = (20, 90, 17)
            argb, mask = random_model(rng, size, with_mask=True)
            model = (None, mask) if op == CARVE else (argb, mask if op == PAINT else None)
            inst = identity_at(at, size, 0, op)
            s, c = _check_call(rules, tmp_path, world, [model], [inst], 2, f"{world_name}, op {op}", dense=True)
            box = (at, tuple(at[i] + size[i] for i in range(3)))
            ds, dc = densemodel.write(solid, colour, box, model[0], model[1], op)
            assert (s == ds).all() and (c == dc).all()


def quarter_forward(transform, size, dst):
    """The exact integer 3 x 4 matrix of cvx_world_copy's transform (mirror X, k quarter turns, flip Y, in that order) on a box of `size`, placed
    at dst; returns it with the destination's size."""
    a = np.eye(4)
    sx, sy, sz = size
    if transform & 4:
        a = np.array([[-1, 0, 0, sx], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]) @ a
    for _ in range(transform & 3):  # (p, q, r) -> (sz - r, q, p)
        a = np.array([[0, 0, -1, sz], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1.0]]) @ a
        sx, sz = sz, sx
    if transform & 8:
        a = np.array([[1, 0, 0, 0], [0, -1, 0, sy], [0, 0, 1, 0], [0, 0, 0, 1.0]]) @ a
    a[:3, 3] += dst
    return a[:3], (sx, sy, sz)


@pytest.mark.parametrize("transform", range(16))
def test_quarter_turns_equal_the_copy(rules, tmp_path, worlds, transform):
    """A source box copied to a scratch model and placed under each of cvx_world_copy's 16 transforms equals tests/copymodel.py's result."""
    world = worlds["terrain"]
    dims, solid, colour, _ = world
    src_min, src_max, dst = (20, 4, 30), (33, 24, 39), (70, 10, 60)
    size = tuple(src_max[i] - src_min[i] for i in range(3))
    argb, mask = densemodel.read(solid, colour, (src_min, src_max))
    assert mask.any() and not mask.all()
    op = (REPLACE, FILL, CARVE, PAINT)[transform % 4]
    forward, dst_size = quarter_forward(transform, size, dst)
    inst = gpu.model_instance(forward, size, 0, op)
    assert all(abs(inst.toModel.m[i][j]) in (0, ONE) for i in range(3) for j in range(3))
    s, c = _check_call(rules, tmp_path, world, [(argb, mask)], [inst], 0, f"transform {transform}")
    placement = dict(srcMin=src_min, srcMax=src_max, dst=dst, transform=transform, op=op, move=0)
    cs, cc = copymodel.apply_copies(solid, colour, [placement])
    assert (s == cs).all() and (c == cc).all(), "the placed model differs from the copy"
    assert ((s != solid) | (c != colour))[dst[0]:dst[0] + dst_size[0], dst[1]:dst[1] + dst_size[1], dst[2]:dst[2] + dst_size[2]].any()


def test_a_wider_box_changes_nothing(rules, tmp_path, worlds):
    """The helper's box is conservative: two voxels wider on every side gives the same world."""
    world = worlds["terrain"]
    dims, solid, colour, _ = world
    rng = np.random.default_rng(5)
    size = (9, 11, 7)
    model = random_model(rng, size)
    results = []
    for widen in (0, 2):
        instances = []
        for k, linear in enumerate((rotation(1, 45), tilt(), 2 * rotation(1, 30), 0.5 * np.eye(3))):
            inst = gpu.model_instance(forward_about_centre(linear, size, (30 + 25 * k, 22, 64)), size, 0, REPLACE)
            for a in range(3):
                inst.boxMin[a] -= widen
                inst.boxMax[a] += widen
            instances.append(inst)
        results.append(modelsmodel.place(solid, colour, [model], as_dicts(instances)))
        if widen:
            _check_call(rules, tmp_path, world, [model], instances, 0, "the wider boxes")
    assert (results[0][0] == results[1][0]).all() and (results[0][1] == results[1][1]).all()
    assert (results[0][0] != solid).any()


# ---- column mode: what the format cannot hold ---------------------------------------------------------------------------------------------------

def test_rule_rejects_what_the_format_cannot_hold(rules, tmp_path):
    """A synthetic 40000-voxel column with its ground voxel solid, under a 1 x 4 x 1 model magnified 8192 times (m[1][1] = 8): the model covers
    [1, 32769).  Filled whole, the column's one run is 32769 voxels, over the limit; clipped by the box to [1, 32767) the run is 32767 voxels
    and is encoded as the builder encodes it."""
    height = 40000
    solid = np.zeros((1, height, 1), dtype=bool)
    solid[0, 0, 0] = True
    colour = np.where(solid, 0xFF010203, 0).astype(np.uint32)
    runs, colours = _builder_column(solid, colour)
    model = (np.arange(0xFF000001, 0xFF000005, dtype=np.uint32).reshape(1, 1, 4), None)
    cases, models = [], []
    for top, over in ((height, True), (32767, False)):
        inst = make_instance([[ONE, 0, 0], [0, 8, 0], [0, 0, ONE]], [0, -8, 0], (0, 1, 0), (1, top, 1), 0, FILL)
        s, c = modelsmodel.place(solid, colour, [model], as_dicts([inst]))
        length = 32769 if over else 32767
        assert s[0, :length, 0].all() and not s[0, length:, 0].any() and (length > 32767) == over
        assert c[0, 1, 0] == 0xFF000001 and c[0, 8192, 0] == 0xFF000001 and c[0, 8193, 0] == 0xFF000002, "every model voxel is a block of 8192"
        want_runs, want_colours = _builder_column(s, c)
        models.append([(over, [((ci & 0xFFFF) | (n << 16)) for ci, n in want_runs], [int(v) for v in want_colours], 0, length)])
        cases.append((height, [(32, runs, colours)], [inst]))
    parts = []
    for dim_y, columns, insts in cases:
        parts += [ruleslib.world_words(dim_y, 1, 1, 1, columns), call_words([model], insts)]
    out = ruleslib.run_cases(rules, "columns", tmp_path, *parts)
    assert out[0] == 1, "a run of 32769 voxels is over the limit"
    over, rc, nc, wmin, wmax = [int(v) for v in out[5:10]]
    results = [[(True, None, None, None, None)], [(bool(over), out[10:10 + rc].tolist(), out[10 + rc:10 + rc + nc].tolist(), wmin, wmax)]]
    assert len(out) == 10 + rc + nc
    _compare(results, models, [(height, 1, 1, 1, None, ((0, 1, 0), None, None, FILL))] * 2)


# ---- read mode ----------------------------------------------------------------------------------------------------------------------------------

def _run_read(rules, tmp_path, ws, size, m, t):
    info = ws.info(0)
    blob, out = tmp_path / "world.bin", tmp_path / "read.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    subprocess.check_call([rules, "read", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), *[str(v) for v in size],
                           *[str(int(v)) for row in m for v in row], *[str(int(v)) for v in t], str(out)])
    raw = out.read_bytes()
    n = size[0] * size[1] * size[2]
    shape = (size[0], size[2], size[1])
    return np.frombuffer(raw[:4 * n], dtype=np.uint32).reshape(shape), np.frombuffer(raw[4 * n:], dtype=np.uint8).reshape(shape).astype(bool)


def test_read_rule_matches_the_model(rules, tmp_path):
    dims = (32, 32, 32)
    solid, colour, ws = _pick_world(np.random.default_rng(1), dims, False)
    try:
        # the identity with a translation: the dense read of a box that sticks out
        at, size = (-3, 5, 20), (20, 30, 15)
        argb, mask = _run_read(rules, tmp_path, ws, size, np.eye(3, dtype=np.int64) * ONE, [a * ONE for a in at])
        want_argb, want_mask = densemodel.read(solid, colour, (at, tuple(at[i] + size[i] for i in range(3))))
        assert want_mask.any() and not want_mask.all()
        assert (argb == want_argb).all() and (mask == want_mask).all()
        # a tilted, scaled sample: toWorld is the rounding of the forward matrix itself, the helper's toModel of the inverse
        forward = forward_about_centre(1.5 * tilt(), size, (16, 12, 16))
        inverse = np.linalg.inv(np.vstack([forward, [0, 0, 0, 1]]))[:3]
        to_world = gpu.model_instance(inverse, dims, 0, REPLACE).toModel
        d = modelsmodel.from_struct(gpu.model_instance(inverse, dims, 0, REPLACE))
        assert np.abs(np.array(d["m"]) / ONE - forward[:, :3]).max() < 1e-4
        argb, mask = _run_read(rules, tmp_path, ws, size, d["m"], d["t"])
        want_argb, want_mask = modelsmodel.read(solid, colour, size, d["m"], d["t"])
        assert want_mask.any() and not want_mask.all() and to_world.m[0][0] == d["m"][0][0]
        assert (argb == want_argb).all() and (mask == want_mask).all()
    finally:
        ws.close()


def test_reading_back_what_was_placed(worlds):
    """The model's read of a placed model through the inverse of its quarter-turn map returns the model."""
    dims, solid, colour, _ = worlds["terrain"]
    size = (7, 9, 5)
    argb, mask = random_model(np.random.default_rng(2), size, with_mask=True, zeros=0.0)
    forward, _ = quarter_forward(9, size, (40, 30, 50))
    inst = gpu.model_instance(forward, size, 0, REPLACE)
    s, c = modelsmodel.place(solid, colour, [(argb, mask)], as_dicts([inst]))
    back = modelsmodel.from_struct(gpu.model_instance(np.linalg.inv(np.vstack([forward, [0, 0, 0, 1]]))[:3], dims, 0, REPLACE))
    got_argb, got_mask = modelsmodel.read(s, c, size, back["m"], back["t"])
    assert (got_mask == mask).all() and (got_argb == np.where(mask, argb, 0)).all()


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------------

def test_instance_from_matrix_is_the_formula():
    """On exactly representable matrices (quarter turns, power-of-two scales, integer and dyadic translations) every step of the formula is
    exact in float64: the helper equals the numpy formula word for word."""
    size = (7, 12, 5)
    checked = 0
    for transform in range(16):
        for scale in (0.25, 0.5, 1.0, 2.0, 4.0):
            forward, _ = quarter_forward(transform, size, (13, -7, 40.5))
            forward = forward.copy()
            forward[:, :3] *= scale
            inst = modelsmodel.from_struct(gpu.model_instance(forward, size, 3, PAINT))
            m, t, lo, hi = modelsmodel.instance_from_matrix(forward, size)
            assert (inst["m"], inst["t"], inst["box_min"], inst["box_max"]) == (m, t, lo, hi), (transform, scale)
            assert inst["model"] == 3 and inst["op"] == PAINT
            # the box holds every world voxel whose image lies inside the model
            d = np.stack(np.meshgrid(*[np.arange(lo[i] - 2, hi[i] + 2) for i in range(3)], indexing="ij"), axis=-1)
            src = modelsmodel.apply_map(m, t, d)
            inside = np.all((src >= 0) & (src < np.array(size)), axis=-1)
            hit = d[inside]
            assert len(hit) and (hit >= np.array(lo)).all() and (hit < np.array(hi)).all()
            checked += 1
    assert checked == 80
    big = modelsmodel.from_struct(gpu.model_instance([[1, 0, 0, 2.0 ** 30 - 4], [0, 1, 0, 0], [0, 0, 1, 0]], size))
    assert big["box_max"][0] == 1 << 30, "clamped"
    for bad in ([[1, 0, 0, 0], [2, 0, 0, 0], [0, 0, 1, 0]], [[np.nan, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[1 / 1024, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]],
                [[1, 0, 0, 3e9], [0, 1, 0, 0], [0, 0, 1, 0]]):
        with pytest.raises(gpu.CvxError):
            gpu.model_instance(bad, size)


# ---- entry points -------------------------------------------------------------------------------------------------------------------------------

def test_calls_fail_cleanly_without_a_context_or_world(rules):
    # a context without a device or world (tests/models_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY, then the helper's CVX_OK
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 42 + [-3] * 5 + [0], codes
    L = gpu.lib()
    handle = C.c_void_p()
    if L.cvx_create(0, C.byref(handle)) == 0:  # (a machine with a device: the world is missing)
        try:
            ctx = object.__new__(gpu.Context)
            ctx._h = handle
            with pytest.raises(gpu.CvxError, match="not been uploaded"):
                ctx.place_models([(np.ones((2, 2, 2), dtype=np.uint32), None)], [identity_at((0, 0, 0), (2, 2, 2))])
            with pytest.raises(gpu.CvxError, match="not been uploaded"):
                ctx.read_model((2, 2, 2), identity_at((0, 0, 0), (2, 2, 2)).toModel)
        finally:
            L.cvx_destroy(handle)


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    inst = [identity_at((0, 0, 0), (2, 2, 2))]
    argb = np.zeros((2, 3, 4), dtype=np.uint32)
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.place_models(ctx, [(argb, np.zeros((2, 3, 5), dtype=bool))], inst)
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.place_models(ctx, [(np.zeros((2, 3), dtype=np.uint32), None)], inst)
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.place_models(ctx, [(None, None)], inst)
    with pytest.raises(ValueError, match="integer array"):
        gpu.Context.place_models(ctx, [(np.zeros((2, 3, 4), dtype=np.float32), None)], inst)
    with pytest.raises(ValueError, match="pair"):
        gpu.Context.place_models(ctx, [argb], inst)
    with pytest.raises(ValueError, match="ModelInstance"):
        gpu.Context.place_models(ctx, [(argb, None)], [dict(op=0)])
    with pytest.raises(ValueError, match="argb_ptr"):
        gpu.Context.place_models_device(ctx, [((2, 2), 0, 0)], inst)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.read_model(ctx, (2, 2), inst[0].toModel)
    with pytest.raises(ValueError, match="ModelMap"):
        gpu.Context.read_model_device(ctx, (2, 2, 2), np.eye(3), 0, 0)
    with pytest.raises(ValueError, match="3 x 4"):
        gpu.model_instance(np.eye(3), (2, 2, 2))
