"""CPU (no GPU needed): the rules behind cvx_world_read_voxels / cvx_world_write_voxels (cpuvox_amd/csrc/cvx_dense.h), compiled for the host
through tests/dense_rules.cpp, against the independent dense model of tests/densemodel.py.

- Column mode: thousands of random columns in small worlds (records with 1..3 runs and listed columns, blocked and column-after-column colour
  layouts, foreign encodings) under random writes (the four ops, with and without a mask, boxes that stick out), against the dense model
  re-encoded with tests/pyworld.py's final_column: runs, colours, worldMin / worldMax and the over-limit rejections must match exactly.  The
  program walks every column twice, with the scalar rule and with the kernels' 64-voxel steps, and fails when the two differ in a word.
- World mode: small random worlds uploaded into a host-only context; the kernels' walk over every column of the call's rectangle gives the
  sub-world blob the write kernel makes, which must equal, byte for byte, the same rectangle of the model's world built on the host.
- Read mode: cvxb::DenseVoxel over boxes inside, across and outside the world against the model.
- The calls without a context / world."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import densemodel
import pyworld
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world, _random_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, CARVE, PAINT, REPLACE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT, gpu.COPY_REPLACE
OPS = {"fill": FILL, "carve": CARVE, "paint": PAINT, "replace": REPLACE}


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("dense_rules", tmp_path_factory.mktemp("dense"))


def _write_words(box_min, argb, mask, op):
    """One write as tests/dense_rules.cpp reads it: boxMin[3] boxSize[3] op hasArgb hasSolid, the argb words, the mask a word per voxel."""
    shape = argb.shape if argb is not None else mask.shape  # (X, Z, Y)
    words = [np.array(list(box_min) + [shape[0], shape[2], shape[1]] + [op, int(argb is not None), int(mask is not None)], dtype=np.int64).astype(np.int32)]
    if argb is not None:
        words.append(np.ascontiguousarray(argb, dtype=np.uint32).ravel().view(np.int32))
    if mask is not None:
        words.append(np.ascontiguousarray(mask).ravel().astype(np.int32))
    return np.concatenate(words)


def _box(box_min, arr):
    return tuple(box_min), (box_min[0] + arr.shape[0], box_min[1] + arr.shape[2], box_min[2] + arr.shape[1])


def random_dense(rng, shape, zeros=0.4, with_mask=None, zero_colours=True):
    """(argb, mask or None) of shape (X, Z, Y): colour words with `zeros` of them 0; under a mask some SET voxels carry the colour word 0."""
    argb = rng.integers(1, 2**32, size=shape, dtype=np.uint64).astype(np.uint32)
    argb[rng.random(shape) < zeros] = 0
    if with_mask is None:
        with_mask = rng.random() < 0.5
    mask = None
    if with_mask:
        mask = rng.random(shape) < 0.5
        if not zero_colours:
            argb[mask & (argb == 0)] = 0xFF112233
    return argb, mask


# ---- column mode -------------------------------------------------------------------------------------------------------------------------------

def _model_columns(solid, colour, box_min, argb, mask, op):
    """Per column (x-major): (over_limit, runs words, colours, worldMin, worldMax) of the model's result re-encoded by the builder's rule."""
    arr = argb if argb is not None else mask
    s, c = densemodel.write(solid, colour, _box(box_min, arr), argb, mask, op)
    gx, dim_y, gz = solid.shape
    out = []
    for x in range(gx):
        for z in range(gz):
            ys = np.nonzero(s[x, :, z])[0][::-1]
            col = pyworld.final_column([(int(y), int(c[x, y, z])) for y in ys], dim_y - 1, 1)
            if col is None:
                out.append((False, [], [], 0, 0))
                continue
            runs, colours, wmin, wmax = col
            over = len(runs) > 65535 or any(n > 32767 for _, n in runs) or any(ci > 32767 for ci, _ in runs)
            out.append((over, [((ci & 0xFFFF) | (n << 16)) for ci, n in runs], list(colours), wmin & 0xFFFF, wmax & 0xFFFF))
    return out


def _run_columns(rules, tmp_path, cases):
    """cases: (dim_y, gx, gz, stride, [(colorsBase, runs, colours)] x-major, (box_min, argb, mask, op)) -> per case, per column (over, runs,
    colours, wmin, wmax)."""
    parts = []
    for dim_y, gx, gz, stride, columns, write in cases:
        parts += [ruleslib.world_words(dim_y, gx, gz, stride, columns), _write_words(*write)]
    out = ruleslib.run_cases(rules, "columns", tmp_path, *parts)
    results, at = [], 0
    for dim_y, gx, gz, *_ in cases:
        per, at = ruleslib.edited_columns(out, at, gx * gz)
        results.append(per)
    assert at == len(out)
    return results


def _compare(results, models, cases):
    bad = [(i, k) for i, (got, want) in enumerate(zip(results, models)) for k, (g, w) in enumerate(zip(got, want))
           if g[0] != w[0] or (not g[0] and list(g[1:]) != list(w[1:]))]
    if bad:
        i, k = bad[0]
        raise AssertionError(f"{len(bad)} columns differ; first: case {i} column {k}: {cases[i][:4]} {cases[i][5][0]} op {cases[i][5][3]}\n"
                             f" got {results[i][k]}\nwant {models[i][k]}")


def _random_world(rng, gx, dim_y, gz):
    """A world of random columns: (solid, colour, [(colorsBase, runs, colours)])."""
    solid = np.zeros((gx, dim_y, gz), dtype=bool)
    colour = np.zeros((gx, dim_y, gz), dtype=np.uint32)
    columns = []
    listed = 0
    for k in range(gx * gz):
        runs, colours, _, dense = _random_column(rng, dim_y)
        x, z = k // gz, k % gz
        colour[x, :, z] = dense
        top = dim_y
        for ci, n in runs:
            if ci >= 0:
                solid[x, top - n:top, z] = True
            top -= n
        columns.append((32 + k * 20000 + int(rng.integers(0, 100)), runs, colours))
        listed += sum(1 for ci, _ in runs if ci >= 0) > 3
    colour[~solid] = 0
    return solid, colour, columns, listed


def test_dense_column_rule_matches_the_dense_model(rules, tmp_path):
    rng = np.random.default_rng(2031)
    cases, models = [], []
    columns_total = listed_like = sticking = masked = zero_set = 0
    ops = [0, 0, 0, 0]
    for _ in range(900):
        dim_y = int(rng.choice([8, 16, 63, 64, 65, 130, 256]))  # below, at and above one and two 64-voxel steps
        gx, gz = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        stride = int(rng.choice([1, 32]))
        solid, colour, columns, listed = _random_world(rng, gx, dim_y, gz)
        listed_like += listed
        lo = [int(rng.integers(-2, gx)), int(rng.integers(-3, dim_y)), int(rng.integers(-2, gz))]
        size = [int(rng.integers(1, gx + 3)), int(rng.integers(1, dim_y + 6)), int(rng.integers(1, gz + 3))]
        argb, mask = random_dense(rng, (size[0], size[2], size[1]))
        op = int(rng.integers(0, 4))
        if op == CARVE and mask is not None and rng.random() < 0.5:
            argb = None
        ops[op] += 1
        masked += mask is not None
        zero_set += mask is not None and argb is not None and bool((mask & (argb == 0)).any())
        sticking += lo[1] < 0 or lo[1] + size[1] > dim_y
        cases.append((dim_y, gx, gz, stride, columns, (lo, argb, mask, op)))
        models.append(_model_columns(solid, colour, lo, argb, mask, op))
        columns_total += gx * gz
    results = _run_columns(rules, tmp_path, cases)
    _compare(results, models, cases)
    assert columns_total > 3000 and listed_like > 100 and sticking > 100 and masked > 300 and zero_set > 200 and min(ops) > 150, \
        (columns_total, listed_like, sticking, masked, zero_set, ops)


def column_cases(dim_y):
    """Named single-column cases (the GPU test uses them too): name -> (arena spans [lo, hi), box y0, argb column, mask column or None, op).
    The argb / mask columns are indexed by y - y0."""
    cases = {}
    third = dim_y // 3
    colours = (0xFF000000 | (np.arange(dim_y, dtype=np.uint32) * 2654435761 >> 8 & 0xFFFFFF)).astype(np.uint32)
    # REPLACE with nothing set over everything the column holds: the zero header
    cases["emptied"] = ([(2, third)], 0, np.zeros(dim_y, dtype=np.uint32), None, REPLACE)
    # arena solid touching the box from above and from below: one merged run, the colours below keep their order
    cases["merged"] = ([(1, third), (2 * third, dim_y - 1)], third, colours[third:2 * third], None, REPLACE)
    # ... and the same with a mask whose set voxels carry the colour word 0
    cases["merged, colour 0"] = ([(1, third), (2 * third, dim_y - 1)], third, np.zeros(third, dtype=np.uint32), np.ones(third, dtype=bool), FILL)
    # an alternating one-voxel pattern over the full height: the most runs a column can have
    alt = np.where(np.arange(dim_y) % 2 == 0, colours, 0).astype(np.uint32)
    cases["alternating"] = ([(0, dim_y)], 0, alt, None, REPLACE)
    cases["alternating carve"] = ([(0, dim_y)], 0, None, np.arange(dim_y) % 2 == 1, CARVE)
    cases["paint over air and solid"] = ([(1, third), (2 * third, dim_y - 1)], 0, colours, None, PAINT)
    return cases


def column_case_world(dim_y, case):
    """(solid, colour) of a 1 x dim_y x 1 world and the write (box_min, argb, mask, op) of one of column_cases."""
    spans, y0, argb, mask, op = case
    solid = np.zeros((1, dim_y, 1), dtype=bool)
    for lo, hi in spans:
        solid[0, lo:hi, 0] = True
    colour = np.where(solid, (0xFF000000 | (np.arange(dim_y, dtype=np.uint32) * 40503 & 0xFFFFFF))[None, :, None], 0).astype(np.uint32)
    return solid, colour, ((0, y0, 0), None if argb is None else argb[None, None, :], None if mask is None else mask[None, None, :], op)


def _builder_column(solid, colour):
    ys = np.nonzero(solid[0, :, 0])[0][::-1]
    col = pyworld.final_column([(int(y), int(colour[0, y, 0])) for y in ys], solid.shape[1] - 1, 1)
    return ([], []) if col is None else (list(col[0]), list(col[1]))


@pytest.mark.parametrize("dim_y", [48, 64, 192, 200])
def test_named_column_cases(rules, tmp_path, dim_y):
    cases, models, names = [], [], []
    for name, case in column_cases(dim_y).items():
        solid, colour, write = column_case_world(dim_y, case)
        runs, colours = _builder_column(solid, colour)
        cases.append((dim_y, 1, 1, 1, [(32, runs, colours)], write))
        models.append(_model_columns(solid, colour, *write))
        names.append(name)
    by_name = dict(zip(names, models))
    # the inputs have the properties they are named for
    assert by_name["emptied"][0] == (False, [], [], 0, 0)
    third = dim_y // 3
    merged = by_name["merged"][0]
    assert [w >> 16 for w in merged[1]] == [1, dim_y - 2, 1] and merged[1][1] & 0xFFFF == 0 and len(merged[2]) == dim_y - 2, "one run through the box"
    assert merged[2][dim_y - 1 - 2 * third:dim_y - 1 - third] == column_cases(dim_y)["merged"][2][::-1].tolist(), "the box's colours in the middle"
    assert by_name["merged, colour 0"][0][2][dim_y - 1 - 2 * third:dim_y - 1 - third] == [0] * third
    assert len(by_name["alternating"][0][1]) == dim_y and len(by_name["alternating carve"][0][1]) == dim_y
    results = _run_columns(rules, tmp_path, cases)
    _compare(results, models, cases)


def test_dense_column_rule_rejects_what_the_format_cannot_hold(rules, tmp_path):
    """A run longer than 32767 voxels, a colour index above 32767 (World.cs:161-259 keeps them in shorts) and more than 65535 runs are over the
    limit, whether the write makes them alone or together with what the arena holds; columns just inside the limits are not.  The tall columns
    are synthetic: 50000 voxels for the run and index cases, and 65536 for the run count -- an alternating column of 65536 voxels has 65536 runs
    and its last solid run the colour index 32767, the one column that is over by its run count alone (at 65535 voxels it fits)."""
    H = 50000

    def arena(*spans, height=H):
        s = np.zeros((1, height, 1), dtype=bool)
        for lo, hi in spans:
            s[0, lo:hi, 0] = True
        c = np.where(s, (0xFF000000 | (np.arange(height, dtype=np.uint32) & 0xFFFFFF))[None, :, None], 0).astype(np.uint32)
        return s, c

    def ones(n):
        return np.full((1, 1, n), 0xFF010203, dtype=np.uint32)

    def alternating(n):  # the top voxel air
        a = np.zeros(n, dtype=np.uint32)
        a[(n - 2)::-2] = 0xFF00FF00
        return a[None, None, :]

    specs = [
        (arena((0, 20000)), ((0, 20000, 0), ones(20000), None, FILL), True),                     # one run of 40000 with the arena's
        (arena((0, 20000)), ((0, 20000, 0), ones(12767), None, FILL), False),                    # 32767: fine
        (arena((0, 20000)), ((0, 20000, 0), ones(12768), None, FILL), True),                     # 32768
        (arena((0, 17000)), ((0, 17001, 0), ones(32768), None, FILL), True),                     # 32768 colours above the arena's run: index 32768
        (arena((0, 17000)), ((0, 17001, 0), ones(32767), None, FILL), False),                    # index 32767: fine
        (arena((0, 40000)), ((0, 20000, 0), None, np.ones((1, 1, 1), dtype=bool), CARVE), False),  # cut in two: 19999 and 20000
        (arena((0, 1)), ((0, 0, 0), np.zeros((1, 1, H), dtype=np.uint32), None, REPLACE), False),  # an air column of 50000: empty, not over
        (arena((0, 1), height=65536), ((0, 0, 0), alternating(65536), None, REPLACE), True),     # 65536 runs, index 32767
        (arena((0, 1), height=65535), ((0, 0, 0), alternating(65535), None, REPLACE), False),    # 65535 runs
    ]
    cases, models = [], []
    for (solid, colour), write, _ in specs:
        runs, colours = _builder_column(solid, colour)
        cases.append((solid.shape[1], 1, 1, 1, [(32, runs, colours)], write))
        models.append(_model_columns(solid, colour, *write))
    want = [over for _, _, over in specs]
    assert [m[0][0] for m in models] == want
    alt = models[7][0]
    assert alt[0] and len(pyworld.final_column([(y, 1) for y in range(65534, -1, -2)], 65535, 1)[0]) == 65536, "65536 runs"
    results = _run_columns(rules, tmp_path, cases)
    assert [r[0][0] for r in results] == want
    _compare(results, models, cases)


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------

def _run_world(rules, tmp_path, ws, write, rect):
    info = ws.info(0)
    blob, wr, out = tmp_path / "world.bin", tmp_path / "write.bin", tmp_path / "sub.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    wr.write_bytes(_write_words(*write).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(wr),
                                    *[str(v) for v in rect], str(out)], text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) over (\d+)", text)
    return out.read_bytes(), int(m.group(1)), int(m.group(2)), int(m.group(3))


def world_cases(dims, rng):
    """Named writes over a world of `dims` (the GPU test uses them too): name -> (box_min, argb, mask, op).  Every op with and without a mask
    (set voxels of colour word 0 under the mask, zeros that are air without one), boxes that stick out on each of the six sides, one wholly
    outside."""
    dx, dy, dz = dims
    cases = {}
    for name, op in OPS.items():
        shape = (dx // 3 + 1, dz // 4 + 3, dy // 2 + 1)
        at = (dx // 5 + 1, dy // 8, dz // 3 - 1)
        argb, mask = random_dense(rng, shape, with_mask=True)
        assert (mask & (argb == 0)).any() and (~mask & (argb != 0)).any()
        cases[f"{name}, mask"] = (at, argb, mask, op)
        argb, _ = random_dense(rng, shape, with_mask=False)
        assert (argb == 0).any()
        cases[f"{name}, no mask"] = (at, argb, None, op)
    cases["carve, mask only"] = ((3, 1, 2), None, rng.random((9, 11, dy // 2)) < 0.6, CARVE)
    small = (7, 6, 9)  # (X, Z, Y)
    for name, at in (("-x", (-3, 5, 4)), ("+x", (dx - 4, 5, 4)), ("-y", (5, -4, 4)), ("+y", (5, dy - 5, 4)), ("-z", (5, 5, -2)), ("+z", (5, 5, dz - 3))):
        cases[f"sticks out {name}"] = (at, random_dense(rng, small, with_mask=False)[0], None, REPLACE)
    cases["sticks out everywhere"] = ((-1, -2, -1), random_dense(rng, (dx + 2, dz + 3, dy + 4), zeros=0.7, with_mask=False)[0], None, FILL)
    cases["wholly outside"] = ((dx + 1, 0, 0), random_dense(rng, small, with_mask=False)[0], None, REPLACE)
    cases["wholly above"] = ((2, dy, 2), random_dense(rng, small, with_mask=False)[0], None, REPLACE)
    return cases


@pytest.mark.parametrize("dims,sparse,level_count,seed", [((32, 32, 32), False, 3, 1), ((16, 64, 32), False, 0, 2), ((32, 256, 32), True, 5, 3)])
def test_written_rectangle_equals_the_model_world(rules, tmp_path, dims, sparse, level_count, seed):
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    cases = world_cases(dims, rng)
    checked = 0
    try:
        for name, (at, argb, mask, op) in cases.items():
            box = _box(at, argb if argb is not None else mask)
            rect = densemodel.rectangle(box, dims, level_count)
            if name.startswith("wholly"):
                assert rect is None
                continue
            if name.startswith("sticks out"):
                assert any(box[0][i] < 0 or box[1][i] > dims[i] for i in range(3))
            s, c = densemodel.write(solid, colour, box, argb, mask, op)
            if not name.startswith("paint") or not sparse:
                assert not (s == solid).all() or not (c == colour).all(), f"{name} changes nothing"
            x, y, z = np.nonzero(s)
            want_ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), c[x, y, z], threads=2)
            try:
                want, _ = want_ws.extract_region(0, *rect)
            finally:
                want_ws.close()
            got, colour_shift, listed, over = _run_world(rules, tmp_path, ws, (at, argb, mask, op), rect)
            assert over == 0
            assert colour_shift == (2 if sparse else 7) and (sparse or listed > 0)
            assert got == want, f"{name}: the sub-world blob of {rect} differs from the model's ({len(got)} vs {len(want)} bytes)"
            checked += 1
    finally:
        ws.close()
    assert checked == len(cases) - 2


# ---- read mode ----------------------------------------------------------------------------------------------------------------------------------

def read_boxes(dims):
    """Boxes of the read tests (the GPU test uses them too): the whole world, one sticking out on all six sides, heights around the wave's 64
    lanes with a bottom that is no multiple of 64, column counts that are no multiple of what a wave packs, one wholly outside."""
    dx, dy, dz = dims
    boxes = {"whole": ((0, 0, 0), dims), "sticks out": ((-2, -3, -1), (dx + 1, dy + 2, dz + 3)), "outside": ((dx, 0, 0), (dx + 3, 4, 5)),
             "5 x 7 columns of 3": ((3, 5, 2), (8, 8, 9))}
    for h in (1, 3, 63, 64, 65, 129):
        boxes[f"height {h}"] = ((1, 7, 2), (4, 7 + h, 7))
    return boxes


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 256, 16), True, 3)])
def test_read_rule_matches_the_dense_model(rules, tmp_path, dims, sparse, seed):
    solid, colour, ws = _pick_world(np.random.default_rng(seed), dims, sparse)
    try:
        info = ws.info(0)
        blob, out = tmp_path / "world.bin", tmp_path / "read.bin"
        blob.write_bytes(ws.storage(0).tobytes())
        for name, (lo, hi) in read_boxes(dims).items():
            size = [hi[i] - lo[i] for i in range(3)]
            subprocess.check_call([rules, "read", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), *[str(v) for v in lo],
                                   *[str(v) for v in size], str(out)])
            raw = out.read_bytes()
            n = size[0] * size[1] * size[2]
            shape = (size[0], size[2], size[1])
            argb = np.frombuffer(raw[:4 * n], dtype=np.uint32).reshape(shape)
            mask = np.frombuffer(raw[4 * n:], dtype=np.uint8).reshape(shape)
            want_argb, want_mask = densemodel.read(solid, colour, (lo, hi))
            if name == "outside":
                assert not want_mask.any()
            elif name in ("whole", "sticks out", "height 129"):
                assert want_mask.any() and not want_mask.all(), f"{name}: solid and air voxels, both"
            assert (argb == want_argb).all() and (mask == want_mask).all(), name
    finally:
        ws.close()


# ---- entry points -------------------------------------------------------------------------------------------------------------------------------

def test_calls_fail_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)
    argb, solid = (C.c_uint32 * 8)(), (C.c_uint8 * 8)()
    assert L.cvx_world_read_voxels(None, lo, hi, argb, solid, None) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    assert L.cvx_world_read_voxels_device(None, lo, hi, argb, solid, None) == -1
    assert L.cvx_world_write_voxels(None, lo, hi, argb, solid, REPLACE, 0, None) == -1
    assert L.cvx_world_write_voxels_device(None, lo, hi, argb, solid, REPLACE, 0, None) == -1
    # a context without a device or world (tests/dense_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 23 + [-3] * 5, codes
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu.h")).read()
    for name in ("cvx_world_read_voxels", "cvx_world_read_voxels_device", "cvx_world_write_voxels", "cvx_world_write_voxels_device"):
        assert name in gpu.EXPORTS and re.search(r"\bint " + name + r"\(", header)
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_read_voxels(h, lo, hi, argb, solid, None) == -3
            assert L.cvx_world_write_voxels(h, lo, hi, argb, solid, REPLACE, 0, None) == -3
        finally:
            L.cvx_destroy(h)


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.write_voxels(ctx, (0, 0, 0), np.zeros((2, 2, 2), dtype=np.uint32), np.zeros((2, 2, 3), dtype=bool))
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.write_voxels(ctx, (0, 0, 0), None, None)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.read_voxels_device(ctx, (0, 0), (1, 1, 1), 0, 0)
